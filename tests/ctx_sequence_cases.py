"""Cases for tests/test_ctx_sequences.py: the clip pool with its oracle values, the operations (one call of one public
entry point on a context, with what it must return), the model of what a call leaves on its context (DESIGN.md section
4, "What a call leaves on its context"), the slips that model is mutated with, and the sequences.  Nothing here touches
the GPU until an operation's `run` is called.

Expected values come from outside the code under test: streams and samples from the CPU oracle, compact blobs from the
host twins (glc_compact_records on the oracle's records, glc_frames_to_compact on the oracle's stream), entries, crops,
verdicts, planner records and row tables from the models of compact_store_cases, crop_cases, store_draw_cases and
compact_decode_cases, the 16-bit narrowing and the integer widening from test_int_pcm's restatements.  The operations of
the five newer families (the store movers, the streaming encode and decode) are built in tests/ctx_sequence_lanes.py.

The model is symbolic: `Op.step(state, mut)` returns a tuple of ints and Sym keys, and never asks the oracle, so the
coverage conditions and the power test cost nothing.  `materialise` turns a Sym into bytes from the pool; a Sym that
only a mutated model can produce ("stale") has no bytes.
"""
from __future__ import annotations

import ctypes as C
import random
import struct

import numpy as np

import compact_decode_cases as K
import compact_store_cases as CS
import conftest as cf
import crop_cases as CC
import roundtrip_cases as RC
import store_draw_cases as S
from conftest import O

SR = 44100
HOP, FRAME = RC.HOP, RC.FRAME
F32 = np.float32
CHS = (1, 2, 3)
EINVAL = -1
NAN_BITS = CC.NAN_BITS
I16_PATTERN = 0x7ABC
CHUNK = 500                      # GLC_FRAMES_PER_CHUNK
PLAN_GROUPS = 2048               # glc_api.hip kPlanGroups
PROBE_COUNTS = (1, 2, 3, 4, 5, 6, 7, 40)      # n_clips a "last" getter is asked with when the model says EINVAL
S16, S32, PF32 = 1, 2, 3

FAMILIES = ("encode", "encode_batch", "encode_dev", "decode", "decode_dev", "decode_batch", "session", "roundtrip",
            "roundtrip_batch", "compact_decode", "crops", "store_encode", "store_draw", "hooks", "switch", "refused",
            "store_compact", "store_join", "store_cut", "stream_encode", "stream_decode")

_g = None


def G():
    """The package (host twins on the CPU side, everything on the GPU side); torch first, so that one HIP runtime is mapped."""
    global _g
    if _g is None:
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        import glc_amd
        _g = glc_amd
    return _g


def narrow(x):
    import test_int_pcm
    return test_int_pcm.narrow(x)


def widen(s, bits):
    import test_int_pcm
    return test_int_pcm.widen(s, bits)


# ------------------------------------------------------------------------------------------ the pool

def per_channel(nf):
    return 513 if nf == 1 else nf * HOP + 100


SMALL = ("one", "tonal9", "tonal9b", "noise5", "mixed13")
FRAMES = {"one": 1, "tonal9": 9, "tonal9b": 9, "noise5": 5, "mixed13": 13, "tonal130": 130, "long1001": 1001,
          "tonal9_i16": 9, "noise5_i16": 5, "tonal9_i32": 9, "noise5_i32": 5}
INT_ITEMS = {"tonal9_i16": ("tonal9", S16, 16), "noise5_i16": ("noise5", S16, 16), "tonal9_i32": ("tonal9", S32, 24),
             "noise5_i32": ("noise5", S32, 24)}


def signal(ch, name):
    if name == "one":
        return RC.chord(SR, ch, 513, seed=11)
    if name == "tonal9":
        return RC.chord(SR, ch, per_channel(9), seed=21)
    if name == "tonal9b":
        return RC.chord(SR, ch, per_channel(9), seed=22)
    if name == "noise5":
        return RC.lcg_noise(per_channel(5) * ch, seed=31)
    if name == "mixed13":       # the pieces of roundtrip_cases.mixed_clip, cut to 13 frames
        return np.concatenate([RC.chord(SR, ch, 5 * HOP, seed=3), RC.lcg_noise(4 * HOP * ch, seed=5), RC.chord(SR, ch, 4 * HOP + 100, seed=4)])
    if name == "tonal130":
        return RC.chord(SR, ch, per_channel(130), seed=41)
    if name == "long1001":
        assert ch == 1
        return RC.chord(SR, 1, per_channel(1001), seed=51)
    raise KeyError(name)


class Item:
    """One clip of the pool; every oracle value is computed on first use and kept."""

    def __init__(self, ch, name):
        self.ch, self.name = ch, name
        self.nf = FRAMES[name]
        self.pc = per_channel(self.nf)
        self.n = self.pc * ch
        self._c = {}

    def _get(self, key, make):
        if key not in self._c:
            self._c[key] = make()
        return self._c[key]

    @property
    def ints(self):
        def make():
            src, fmt, bits = INT_ITEMS[self.name]
            v = np.rint(signal(self.ch, src).astype(np.float64) * (2 ** (bits - 1) - 1))
            return v.astype(np.int16 if fmt == S16 else np.int32)
        return self._get("ints", make)

    @property
    def x(self):
        def make():
            if self.name in INT_ITEMS:
                return np.ascontiguousarray(widen(self.ints, INT_ITEMS[self.name][2]), F32)
            return np.ascontiguousarray(signal(self.ch, self.name), F32)
        x = self._get("x", make)
        assert x.size == self.n and RC.frames_of(self.pc) == self.nf
        return x

    @property
    def glc(self):
        return self._get("glc", lambda: O.encode(self.x, SR, self.ch).glc)

    @property
    def dec(self):
        return self._get("dec", lambda: O.decode(self.glc)[0])

    @property
    def dec16(self):
        return self._get("dec16", lambda: narrow(self.dec))

    @property
    def parsed(self):
        return self._get("parsed", lambda: cf.parse_glc(self.glc))

    @property
    def info(self):
        """(n_frames, n_raw_frames, total_nnz, serialized_bytes): what glc_roundtrip_last_info must give."""
        fr = self.parsed["frames"]
        return (len(fr), sum(f["raw"] is not None for f in fr), sum(len(l[0]) for f in fr for l in f["lists"]), len(self.glc))

    @property
    def taps(self):
        return self._get("taps", lambda: O.encode_range_records(self.x, 0, self.pc, self.n, SR, self.ch, 0, self.nf, taps=True))

    @property
    def records(self):
        return self.taps[0]

    @property
    def coeffs(self):
        return self.taps[1].coeffs

    @property
    def blob_enc(self):
        """The blob the ENCODER's store holds: the host twin of the packing on the oracle's records."""
        return self._get("blob_enc", lambda: np.ascontiguousarray(G().compact_records(self.records, self.ch), np.uint8))

    @property
    def blob(self):
        """The blob of the oracle's stream (glc_frames_to_compact): what a host uploads into a store."""
        def make():
            g = G()
            return np.frombuffer(g.frames_to_compact(g.EncodedAudio.from_bytes(self.glc)), np.uint8).copy()
        return self._get("blob", make)


class Damaged:
    """One of the two damaged stereo blobs of crop_cases / compact_decode_cases, unchanged, with what it decodes AS."""

    def __init__(self, name):
        self.ch, self.name = 2, name
        self.base = CC.stereo_stream()
        self.nf = len(self.base)
        self.pc = self.nf * HOP
        self.n = K.n_samples_of(2, self.nf)
        if name == "bad_header":
            self.buf, _ = K.pack(2, self.base, magic=K.MAGIC ^ 0x100)
            self.as_frames = K.emptied(2, self.base, all_rows=True)
            self.bad_rows = None
        elif name == "bad_row7":
            self.buf, _ = K.pack(2, CC.with_bad_list(self.base, 7))
            self.as_frames = K.emptied(2, CC.with_bad_list(self.base, 7), rows=[7])
            self.bad_rows = (7,)
        else:                    # the undamaged stream the two are made from
            self.buf, _ = K.pack(2, self.base)
            self.as_frames = self.base
            self.bad_rows = ()
        self.blob = self.buf     # the entry names the whole buffer, as the crop tests do
        self._dec = None

    @property
    def dec(self):
        if self._dec is None:
            g = G()
            buf, nbytes = K.pack(2, self.as_frames)
            stream = g.EncodedAudio.from_compact(SR, self.n, 2, [buf[:nbytes]])
            self._dec = O.decode(stream.to_bytes())[0]
            assert self._dec.size == self.n
        return self._dec

    def status(self, first_row=0, rows=None):
        """The status words of rows [first_row, first_row + rows) of this blob (include/glc.h)."""
        rows = self.nf * 2 if rows is None else rows
        if self.bad_rows is None:
            return (K.BAD_HEADER, rows, first_row)
        hit = [r for r in self.bad_rows if first_row <= r < first_row + rows]
        return (K.NOT_CANONICAL, len(hit), hit[0]) if hit else (0, 0, 0)


_items = {}
DAMAGED = ("bad_header", "bad_row7", "crafted")


def item(ch, name):
    key = (ch, name)
    if key not in _items:
        _items[key] = Damaged(name) if name in DAMAGED else Item(ch, name)
    return _items[key]


def K_ID(ch, name):
    """The caller's stream id of the from_parts copies of a pool stream."""
    return 0x5EED00 + 16 * ch + sorted(FRAMES).index(name)


def fingerprint(ch, name):
    """What decode_prepare compares besides the id.  The model only asks whether two of them differ."""
    return (ch, FRAMES[name], name)          # same shape, other content: the pair count differs


# ------------------------------------------------------------------------------------------ symbols

def sym(*a):
    return ("sym",) + a


def is_sym(v):
    return isinstance(v, tuple) and len(v) > 0 and v[0] == "sym"


def fill_batch(shape, planar, arrays, ch, dtype=np.uint32, pattern=NAN_BITS):
    want = np.full(shape, pattern, dtype)
    for i, a in enumerate(arrays):
        a = np.ascontiguousarray(a).view(dtype).reshape(-1, ch)
        if planar:
            want[i, :ch, :a.shape[0]] = a.T
        else:
            want[i, :a.shape[0], :ch] = a
    return want


def untrimmed_slice(it, lo, hi, fmt="f32"):
    """Positions [lo, hi) of the un-trimmed stream that the oracle knows: those inside [512, 512 + n) -> (offset of the
    first known position from lo, the known samples)."""
    d = it.dec if fmt == "f32" else it.dec16
    a, b = max(lo, 512), min(hi, 512 + it.n)
    return a - lo, d[a - 512:b - 512]


def materialise(v, assets=None):
    """Bytes (or a plain value) of one expected element."""
    if not is_sym(v):
        return v
    kind = v[1]
    if kind == "einval":
        return "EINVAL"
    if kind == "status":
        return tuple(tuple(w) for w in v[2])
    if kind == "dec":
        _, _, ch, name, fmt = v
        it = item(ch, name)
        return (it.dec if fmt == "f32" else it.dec16).tobytes()
    if kind == "glc":
        return item(v[2], v[3]).glc
    if kind == "glcs":
        return tuple(item(v[2], n).glc for n in v[3])
    if kind == "records":
        return item(v[2], v[3]).records.tobytes()
    if kind == "coeffs":
        return np.ascontiguousarray(item(v[2], v[3]).coeffs, F32).tobytes()
    if kind == "blob_enc":
        return item(v[2], v[3]).blob_enc.tobytes()
    if kind == "x":
        return item(v[2], v[3]).x.tobytes()
    if kind == "window":                     # a slice of the un-trimmed stream
        _, _, ch, name, lo, hi, fmt = v
        return untrimmed_slice(item(ch, name), lo, hi, fmt)[1].tobytes()
    if kind == "packed":                     # decode_batch: the streams' samples back to back
        _, _, ch, names, fmt = v
        return b"".join((item(ch, n).dec if fmt == "f32" else item(ch, n).dec16).tobytes() for n in names)
    if kind == "batch":                      # a NaN-pattern tensor with the clips' decoded samples in it
        _, _, ch, names, planar, shape = v
        return fill_batch(shape, planar, [item(ch, n).dec for n in names], ch).tobytes()
    if kind == "crops":
        _, _, ch, sels, planar, shape = v
        return CC.want_crops(shape, planar, 0, ch, [(item(ch, n).dec, s, l) if n else (np.zeros(l * ch, F32), 0, l) for n, s, l in sels]).tobytes()
    if kind == "rtinfo":
        return item(v[2], v[3]).info
    if kind == "rtbinfo":
        return tuple(item(v[2], n).info for n in v[3])
    if kind == "uid":                        # a library-made id: known once the assets exist
        return assets.streams[(v[2], v[3], "lib")].stream_id
    if kind == "store":                      # (entry rows, arena image, cursor) of a store the encoder fills
        _, _, ch, calls, arena_bytes = v
        return store_expect(ch, calls, arena_bytes)
    if kind == "tables":
        _, _, first, rows = v
        t = K.tables(2, item(2, "crafted").base)
        return tuple(np.ascontiguousarray(a[first:first + rows]).tobytes() for a in t)
    if kind == "plan":
        return plan_expect(assets, *v[2:])
    if kind == "pack":
        return pack_expect(v[2], v[3])
    import ctx_sequence_lanes as LN          # the symbols of the newer families
    return LN.materialise(v, assets)


def records_specified(got: bytes, ch, name):
    """Frame records as the device left them in a buffer prefilled with 0xA5, with the bytes include/glc.h leaves
    unspecified - the reserved word, the header's padding, the upper half of a compressed frame's payload rows - set to the
    oracle's where they are untouched (0xA5) or already the oracle's; anything else there stays and fails the comparison."""
    it = item(ch, name)
    want = it.records.reshape(it.nf, -1)
    a = np.frombuffer(got, np.uint8).reshape(it.nf, -1).copy()
    hdr = RC.record_layout(ch)[0]
    free = np.zeros(a.shape, bool)
    free[:, 4:8] = True
    free[:, 8 + 8 * ch:hdr] = True
    for f in np.flatnonzero(it.taps[1].is_raw == 0):
        for c in range(ch):
            free[f, hdr + c * 4096 + 2048:hdr + (c + 1) * 4096] = True
    ok = free & ((a == 0xA5) | (a == want))
    a[ok] = want[ok]
    return a.tobytes()


def blob_counts(blob):
    _, _, _, n_pairs, n_raw, nbytes = struct.unpack_from("<IIQQQQ", blob, 0)
    return n_pairs, n_raw, nbytes


def store_expect(ch, calls, arena_bytes):
    """compact_store_cases.store_model over the host twins' blobs, call after call through one cursor."""
    cursor, rows, img = 0, [], np.full(arena_bytes, CS.SENTINEL, np.uint8)
    for names in calls:
        blobs = [(item(ch, n).blob_enc,) + blob_counts(item(ch, n).blob_enc)[:2] for n in names]
        assert all(b.size == blob_counts(b)[2] and b.size % 64 == 0 for b, _, _ in blobs)
        entries, bl, cursor = CS.store_model(None, None, cursor, arena_bytes, blobs=blobs)
        img = CS.arena_image(arena_bytes, entries, bl, image=img)
        rows.append(CS.entry_rows(entries).tobytes())
    return tuple(rows), img.tobytes(), cursor


# ------------------------------------------------------------------------------------------ the model

FORGETTING = ("decode_batch", "roundtrip", "roundtrip_batch", "compact_decode", "crops", "store_encode", "store_draw", "hooks",
              "stream_encode", "stream_decode")
MOVERS = ("store_compact", "store_join", "store_cut")
MUTATIONS = tuple(f"{f}_keeps_resident" for f in FORGETTING) + (
    "plan_ignores_row_begin", "plan_ignores_M", "variant_switch_keeps_plan",
    "resident_ignores_pair_count", "refused_clears_last_status", "refused_closes_nothing", "clean_status_ored",
    "store_compact_forgets", "store_join_forgets", "store_cut_forgets", "mover_clears_last_status", "stream_decode_leaves_last_status",
    "empty_push_keeps_last_status", "refused_push_moves_lane", "forgetting_call_resets_lanes")

# "a growing reserve keeps the plan" is modelled (m_reserve) but is no member of MUTATIONS: no sequence of public calls can
# show it.  reserve_d1_plan grows only for a launch of more units than any before it; a kept plan belongs to the resident
# stream, whose launches need the units they needed when the plan was made; every other caller of the reserve forgets the
# stream in the same call.  test_the_growing_reserve_slip_is_unobservable pins that reasoning against the sequences.
EQUIVALENT_MUTATIONS = ("growing_reserve_keeps_plan",)

ORDER = {0: "rank", 2: "rank", 3: "rank", 4: "rank", 5: "cu", 6: "rot", 1: "rows"}


class State:
    """What a context carries from call to call, as far as a caller can observe it."""

    def __init__(self):
        self.res_id = 0          # id of the resident stream
        self.res_fp = None       # its fingerprint
        self.rows = None         # the content whose rows the device holds for it
        self.plan_uid = 0        # the kept D1 plan: the id, launch and content it was made for
        self.plan_rb = self.plan_M = 0
        self.plan_of = None
        self.groups = 0          # units the plan workspace holds
        self.variant = 0
        self.sess = None         # open session: dict(ch, name, next, fmt)
        self.rt = self.rtb = self.cd = None
        # the lanes of the open stream encoders / decoders: (ch, "host" | "dev", lane) -> dict(name: the clip, at: samples
        # per channel received / frames done, finished, segs: the host segments not handed over yet).  Only an accepted
        # push or a reset of that lane changes a lane; no other call does, whatever else it forgets.
        self.enc, self.dec = {}, {}
        self.pending = None      # what the last lane operation's `step` decided to push: its `run` carries it out

    def tail(self):
        return (self.rt if self.rt is not None else sym("einval"), self.rtb if self.rtb is not None else sym("einval"),
                self.cd if self.cd is not None else sym("einval"), self.res_id)


def m_reserve(st, mut, nf, ch):
    if st.variant == 1:
        return
    units = -(-nf // 8) * ch
    want = max(ch, min(max(PLAN_GROUPS, ch), units))
    if want > st.groups:
        st.groups = want
        if mut != "growing_reserve_keeps_plan":
            st.plan_uid = 0


def m_prepare(st, mut, ch, name, uid):
    m_reserve(st, mut, FRAMES[name], ch)
    fp = fingerprint(ch, name)
    same = st.res_fp == fp or (mut == "resident_ignores_pair_count" and st.res_fp is not None and st.res_fp[:2] == fp[:2])
    if st.res_id != 0 and st.res_id == uid and same:
        return
    st.res_id, st.res_fp, st.rows, st.plan_uid = uid, fp, (ch, name), 0


def m_d1(st, mut, row_begin, M):
    """One D1 launch on the prepared stream -> the content it computes, or a "stale" symbol."""
    ch = st.rows[0]
    planned = st.variant != 1
    fresh = (st.rows, row_begin, M, ORDER[st.variant])
    one_batch = planned and -(-(M // ch) // 8) * ch <= st.groups
    reuse = (one_batch and st.plan_uid == st.res_id and st.plan_uid != 0 and
             (st.plan_rb == row_begin or mut == "plan_ignores_row_begin") and (st.plan_M == M or mut == "plan_ignores_M"))
    used = st.plan_of if reuse else fresh
    if planned:
        if not reuse:
            st.plan_of = fresh
        st.plan_uid, st.plan_rb, st.plan_M = (st.res_id if one_batch else 0), row_begin, M
    return st.rows if used == fresh else ("stale", used, fresh)


def m_forget(st, mut, family):
    """The rule of the round-trip and store families: no session survives, no stream is resident, the plan is another launch's."""
    st.plan_of = ("other", family)
    if mut == "forgetting_call_resets_lanes":
        st.enc.clear()
        st.dec.clear()
    if mut == f"{family}_keeps_resident":
        return
    st.sess, st.res_id, st.plan_uid = None, 0, 0


def content_sym(got, fmt):
    if got[0] == "stale":
        return sym("stale", got)
    return sym("dec", got[0], got[1], fmt)


# ------------------------------------------------------------------------------------------ operations

class Op:
    def __init__(self, name, family, ch, size, step, run, device_only=False, clips=(), calls=()):
        self.name, self.family, self.ch, self.size, self.step, self.run, self.device_only = name, family, ch, size, step, run, device_only
        self.clips = tuple(clips)        # the pool clips the call works on
        self.calls = tuple(calls)        # the entry points of include/glc.h that `run` calls
        self.lane = None                 # ("enc" | "dec", key into State.enc / State.dec) of a lane operation

    def __repr__(self):
        return self.name


class Env:
    """What `run` works with: the context under test and the shared assets."""

    def __init__(self, g, torch, ctx, assets):
        self.g, self.torch, self.ctx, self.A = g, torch, ctx, assets
        self.h = ctx._h
        self.keep = []
        self.sessions = {}       # the open stream encoders / decoders (ctx_sequence_lanes.session)
        self.st = None           # the model's state of this context: a lane operation's `run` reads State.pending

    def close(self):
        """The sessions go before their context."""
        import ctx_sequence_lanes as LN
        LN.close_sessions(self)

    def ready(self):
        """Everything torch has queued (fills of fresh buffers) is done; the context's own stream is not waited for."""
        self.torch.cuda.current_stream().synchronize()


def vp(t):
    return C.c_void_p(t.data_ptr())


def dfull(torch, shape, value, dtype):
    """A filled device tensor, copied up from the host: the copy is over when this returns, whatever stream reads next."""
    return torch.from_numpy(np.full(shape, value, dtype)).cuda()


def nan_f32(torch, n):
    return torch.from_numpy(np.full(n, NAN_BITS, np.uint32).view(F32)).cuda()


def pat_i16(torch, n):
    return torch.from_numpy(np.full(n, I16_PATTERN, np.int16)).cuda()


def payload_and_guard(t, n, pattern=NAN_BITS):
    """(the first n elements' bytes, whether everything behind them is still the pattern)."""
    a = t.cpu().numpy().reshape(-1)
    w = a.view(np.uint32) if a.dtype == np.float32 else a
    return a[:n].tobytes(), bool(np.all(w[n:] == (pattern if a.dtype == np.float32 else I16_PATTERN)))


def host_f32(n, margin=8):
    return np.full(n + margin, NAN_BITS, np.uint32).view(F32)


def host_i16(n, margin=8):
    return np.full(n + margin, I16_PATTERN, np.int16)


def host_payload(buf, n):
    w = buf.view(np.uint32) if buf.dtype == np.float32 else buf
    return buf[:n].tobytes(), bool(np.all(w[n:] == (NAN_BITS if buf.dtype == np.float32 else I16_PATTERN)))


def done(*vals):
    return lambda: tuple(vals)


def layout(g, n, ch, planar, t, lens=None, keep=None):
    """The glc_clip_layout of a dense tensor (n, ch, t) / (n, t, ch)."""
    lay = g._lib.GlcClipLayout(n, ch, 1 if planar else 0, ch * t, t if planar else 0, t, None)
    if lens is not None:
        arr = (C.c_uint64 * max(n, 1))(*lens)
        lay.lengths = C.cast(arr, C.POINTER(C.c_uint64))
        keep.append(arr)
    return lay


def batch_in(env, ch, names, planar):
    """The clips of a batch in a NaN-padded (B, C, T) / (B, T, C) device tensor."""
    its = [item(ch, n) for n in names]
    t = max(i.pc for i in its)
    shape = (len(its), ch, t) if planar else (len(its), t, ch)
    words = fill_batch(shape, planar, [i.x for i in its], ch)
    return env.torch.from_numpy(words.view(F32)).cuda(), t, [i.pc for i in its], shape


def frames_to_bytes(env, handle):
    ea = env.g.EncodedAudio(handle)
    return ea.to_bytes()


# ---- builders: each returns an Op ----

def op_encode(ch, name, how="f32", size="small"):
    it = item(ch, name)

    def step(st, mut):
        return (0, sym("glc", ch, name))

    def run(env):
        out = C.c_void_p()
        L = env.g.lib
        if how == "f32":
            rc = L.glc_encode(env.h, it.x.ctypes.data, it.n, ch, C.byref(out))
        elif how == "int":
            _, fmt, bits = INT_ITEMS[name]
            rc = L.glc_encode_int(env.h, it.ints.ctypes.data, fmt, bits, it.n, ch, C.byref(out))
        else:
            cb = env.g._lib.FRAMES_HOOK(lambda user, view, f0, f1: 0)
            rc = L.glc_encode_hooked(env.h, it.x.ctypes.data, it.n, ch, cb, None, C.byref(out))
        return done(rc, frames_to_bytes(env, out.value) if rc == 0 else b"")
    return Op(f"encode-{how}({name},{ch}ch)", "encode", ch, size, step, run, clips=(name,),
              calls=({"f32": "glc_encode", "int": "glc_encode_int", "hooked": "glc_encode_hooked"}[how],))


def op_encode_batch(ch, names, how="f32", size="small"):
    its = [item(ch, n) for n in names]

    def step(st, mut):
        return (0, sym("glcs", ch, tuple(names)))

    def run(env):
        n = len(its)
        L = env.g.lib
        outs = (C.c_void_p * n)()
        lens = (C.c_uint64 * n)(*[i.n for i in its])
        if how == "f32":
            ptrs = (C.c_void_p * n)(*[i.x.ctypes.data for i in its])
            rc = L.glc_encode_batch(env.h, ptrs, lens, n, ch, outs)
        else:
            _, fmt, bits = INT_ITEMS[names[0]]
            ptrs = (C.c_void_p * n)(*[i.ints.ctypes.data for i in its])
            rc = L.glc_encode_batch_int(env.h, ptrs, fmt, bits, lens, n, ch, outs)
        return done(rc, tuple(frames_to_bytes(env, outs[i]) for i in range(n)) if rc == 0 else ())
    return Op(f"encode_batch-{how}({len(names)}x{names[0]}..,{ch}ch)", "encode_batch", ch, size, step, run, clips=names,
              calls=("glc_encode_batch" if how == "f32" else "glc_encode_batch_int",))


def op_encode_dev(ch, name, what, size="small"):
    it = item(ch, name)
    rec_bytes = it.nf * O.record_bytes(ch)

    def step(st, mut):
        if what in ("range", "quantize"):
            return (0, sym("records", ch, name), True)
        if what == "mdct":
            return (0, sym("coeffs", ch, name), True)
        if what == "compact":
            return (0, sym("blob_enc", ch, name), True)
        if what == "frames":
            return (0, sym("glc", ch, name))
        return (0, sym("x", ch, name), True)          # widen

    def run(env):
        t, L, A = env.torch, env.g.lib, env.A
        if what == "range":
            out = dfull(t, rec_bytes + 64, 0xA5, np.uint8)
            rc = L.glc_encode_range_device(env.h, vp(A.x(ch, name)), 0, it.pc, it.n, ch, 0, it.nf, vp(out), None)
            return lambda: (rc, out[:rec_bytes].cpu().numpy().tobytes(), bool((out[rec_bytes:] == 0xA5).all()))
        if what == "quantize":
            f = L.glc_debug_quantize_device
            f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint16, C.c_uint64,
                                              C.c_uint64, C.c_void_p]
            out = dfull(t, rec_bytes + 64, 0xA5, np.uint8)
            rc = f(env.h, vp(A.coeffs(ch, name)), vp(A.x(ch, name)), 0, it.pc, it.n, ch, 0, it.nf, vp(out))
            return lambda: (rc, out[:rec_bytes].cpu().numpy().tobytes(), bool((out[rec_bytes:] == 0xA5).all()))
        if what == "mdct":
            n = it.nf * ch * HOP
            out = nan_f32(t, n + 8)
            rc = L.glc_mdct_forward_device(env.h, vp(A.x(ch, name)), 0, it.pc, it.n, ch, 0, it.nf, vp(out))
            return lambda: (rc,) + payload_and_guard(out, n)
        if what == "compact":
            cap = int(L.glc_compact_bound(ch, it.nf))
            out = dfull(t, cap + 64, 0xA5, np.uint8)
            info = env.g._lib.GlcCompactInfo()
            rc = L.glc_compact_device_records(env.h, vp(A.records(ch, name)), it.nf, ch, vp(out), cap, C.byref(info))
            nb = int(info.bytes)
            return lambda: (rc, out[:nb].cpu().numpy().tobytes(), bool((out[nb:] == 0xA5).all()))
        if what == "frames":
            out = C.c_void_p()
            rc = L.glc_frames_from_device_records(env.h, vp(A.records(ch, name)), it.nf, it.n, ch, C.byref(out))
            return done(rc, frames_to_bytes(env, out.value) if rc == 0 else b"")
        _, fmt, bits = INT_ITEMS[name]
        out = nan_f32(t, it.n + 8)
        rc = L.glc_pcm_widen_device(env.h, vp(A.ints(ch, name)), fmt, bits, it.n, vp(out))
        return lambda: (rc,) + payload_and_guard(out, it.n)
    sync = what in ("compact", "frames")
    call = {"range": "glc_encode_range_device", "quantize": "glc_debug_quantize_device", "mdct": "glc_mdct_forward_device",
            "compact": "glc_compact_device_records", "frames": "glc_frames_from_device_records", "widen": "glc_pcm_widen_device"}[what]
    return Op(f"{what}-device({name},{ch}ch)", "hooks" if what == "quantize" else "encode_dev", ch, size, step, run, device_only=not sync, clips=(name,),
              calls=(call,))


def uid_of(ch, name, ident):
    """ident: "lib" (the library's own id), "k1" / "k2" (two from_parts copies with one caller id), or ("as", other): a
    from_parts copy of `name` that carries the id of `other`."""
    if ident == "lib":
        return sym("uid", ch, name)
    if isinstance(ident, tuple):
        return K_ID(ch, ident[1])
    return K_ID(ch, name)


def op_decode(ch, name, ident="lib", fmt="f32", size="small"):
    it = item(ch, name)
    M = it.nf * ch

    def step(st, mut):
        st.sess = None
        m_prepare(st, mut, ch, name, uid_of(ch, name, ident))
        return (0, it.n, content_sym(m_d1(st, mut, 0, M), fmt), True)

    def run(env):
        s = env.A.streams[(ch, name, ident)]
        buf = host_f32(it.n) if fmt == "f32" else host_i16(it.n)
        got = C.c_uint64()
        fn = env.g.lib.glc_decode if fmt == "f32" else env.g.lib.glc_decode_i16
        rc = fn(env.h, s._h, buf.ctypes.data, it.n, C.byref(got))
        return done(rc, int(got.value), *host_payload(buf, it.n))
    tag = ident if isinstance(ident, str) else f"id-of-{ident[1]}"
    return Op(f"decode-{fmt}({name}/{tag},{ch}ch)", "decode", ch, size, step, run, clips=(name,),
              calls=("glc_decode" if fmt == "f32" else "glc_decode_i16",))


def op_decode_resident(ch, name):
    it = item(ch, name)

    def step(st, mut):
        if st.res_id != K_ID(ch, name):
            return (EINVAL, 0, b"", True)
        st.sess = None
        return (0, it.n, content_sym(m_d1(st, mut, 0, it.nf * ch), "f32"), True)

    def run(env):
        buf = host_f32(it.n)
        got = C.c_uint64()
        rc = env.g.lib.glc_decode_resident(env.h, K_ID(ch, name), buf.ctypes.data, it.n, C.byref(got))
        if rc != 0:
            return done(rc, 0, b"", host_payload(buf, 0)[1])
        return done(rc, int(got.value), *host_payload(buf, it.n))
    return Op(f"decode_resident({name},{ch}ch)", "decode", ch, "small", step, run, clips=(name,), calls=("glc_decode_resident",))


def op_decode_device(ch, name):
    """glc_decode_device: the oracle knows the trimmed window of the un-trimmed stream; it is compared, with the start
    and length the call reports, and the pattern behind the capacity."""
    it = item(ch, name)
    total = (it.nf + 1) * HOP * ch

    def step(st, mut):
        st.sess = None
        m_prepare(st, mut, ch, name, sym("uid", ch, name))
        return (0, 512, it.n, content_sym(m_d1(st, mut, 0, it.nf * ch), "f32"), True)

    def run(env):
        out = nan_f32(env.torch, total + 8)
        start, n = C.c_uint64(), C.c_uint64()
        rc = env.g.lib.glc_decode_device(env.h, env.A.streams[(ch, name, "lib")]._h, vp(out), total, C.byref(start), C.byref(n))

        def fin():
            a = out.cpu().numpy()
            return (rc, int(start.value), int(n.value), a[512:512 + it.n].tobytes(), bool(np.all(a[total:].view(np.uint32) == NAN_BITS)))
        return fin
    return Op(f"decode_device({name},{ch}ch)", "decode_dev", ch, "small", step, run, device_only=True, clips=(name,), calls=("glc_decode_device",))


def op_decode_range(ch, name, h0, h1, fmt="f32"):
    """Hops [h0, h1) of the un-trimmed stream, a proper sub-range that lies inside the samples the oracle knows."""
    it = item(ch, name)
    lo, hi = h0 * HOP * ch, h1 * HOP * ch
    assert 0 <= h0 < h1 <= it.nf + 1 and (h0, h1) != (0, it.nf + 1) and hi <= 512 + it.n
    off = max(512 - lo, 0)

    def step(st, mut):
        st.sess = None
        m_prepare(st, mut, ch, name, sym("uid", ch, name))
        got = []
        if h0:
            got.append(m_d1(st, mut, (h0 - 1) * ch, ch))
        f_end = min(h1, it.nf)
        if f_end > h0:
            got.append(m_d1(st, mut, h0 * ch, (f_end - h0) * ch))
        bad = [x for x in got if x[0] == "stale"]
        return (0, sym("stale", bad[0]) if bad else sym("window", ch, name, lo, hi, fmt), True)

    def run(env):
        n = hi - lo
        s = env.A.streams[(ch, name, "lib")]
        if fmt == "f32":
            out = nan_f32(env.torch, n + 8)
            rc = env.g.lib.glc_decode_range_device(env.h, s._h, h0, h1, vp(out), n)
        else:
            out = pat_i16(env.torch, n + 8)
            rc = env.g.lib.glc_decode_range_device_i16(env.h, s._h, h0, h1, vp(out), n)

        def fin():
            a = out.cpu().numpy()
            w = a.view(np.uint32) if fmt == "f32" else a
            return (rc, a[off:n].tobytes(), bool(np.all(w[n:] == (NAN_BITS if fmt == "f32" else I16_PATTERN))))
        return fin
    return Op(f"decode_range-{fmt}({name},{h0}..{h1},{ch}ch)", "decode_dev", ch, "small", step, run, device_only=True, clips=(name,),
              calls=("glc_decode_range_device" if fmt == "f32" else "glc_decode_range_device_i16",))


def op_imdct(ch, name, f0, f1, size="small"):
    """glc_imdct_device of frames [f0, f1), a proper sub-range, held to the oracle through the overlap-add hook: hops
    f0 + 1 .. f1 - 1 need exactly those blocks."""
    it = item(ch, name)
    assert 0 <= f0 and f0 + 2 <= f1 <= it.nf and (f0, f1) != (0, it.nf)
    h0, h1 = f0 + 1, f1
    lo, hi = h0 * HOP * ch, h1 * HOP * ch
    assert lo >= 512 and hi <= 512 + it.n

    def step(st, mut):
        st.sess = None
        m_prepare(st, mut, ch, name, sym("uid", ch, name))
        got = m_d1(st, mut, f0 * ch, (f1 - f0) * ch)
        return (0, 0, sym("stale", got) if got[0] == "stale" else sym("window", ch, name, lo, hi, "f32"), True)

    def run(env):
        t, L = env.torch, env.g.lib
        nb = (f1 - f0) * ch * FRAME
        blocks = nan_f32(t, nb)
        rc = L.glc_imdct_device(env.h, env.A.streams[(ch, name, "lib")]._h, f0, f1, vp(blocks))
        f = L.glc_debug_overlap_add_device
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_uint16, C.c_uint64, C.c_uint64,
                                          C.c_void_p, C.c_uint64]
        out = nan_f32(t, hi - lo + 8)
        rc2 = f(env.h, vp(blocks), f0, f1 - f0, it.nf, ch, h0, h1, vp(out), hi - lo) if rc == 0 else EINVAL
        env.keep.append(blocks)      # queued work still reads it: it must not go back to torch's allocator yet
        return lambda: (rc, rc2) + payload_and_guard(out, hi - lo)
    return Op(f"imdct_device+overlap_add({name},{f0}..{f1},{ch}ch)", "decode_dev", ch, size, step, run, device_only=True, clips=(name,),
              calls=("glc_imdct_device", "glc_debug_overlap_add_device"))


def op_decode_batch(ch, names, fmt="f32", size="small"):
    its = [item(ch, n) for n in names]
    total = sum(i.n for i in its)

    def step(st, mut):
        st.sess = None           # a batch decode clears by hand; a stream with a round to itself is prepared like any other
        if mut != "decode_batch_keeps_resident":
            st.res_id, st.plan_uid = 0, 0
        elif len(names) == 1:
            m_prepare(st, mut, ch, names[0], sym("uid", ch, names[0]))
        st.plan_of = ("other", "decode_batch")
        return (0, tuple(np.cumsum([0] + [i.n for i in its]).tolist()), sym("packed", ch, tuple(names), fmt), True)

    def run(env):
        n = len(its)
        hs = (C.c_void_p * n)(*[env.A.streams[(ch, nm, "lib")]._h for nm in names])
        offs = (C.c_uint64 * (n + 1))()
        buf = host_f32(total) if fmt == "f32" else host_i16(total)
        fn = env.g.lib.glc_decode_batch if fmt == "f32" else env.g.lib.glc_decode_batch_i16
        rc = fn(env.h, hs, n, buf.ctypes.data, total, offs)
        return done(rc, tuple(int(v) for v in offs), *host_payload(buf, total))
    return Op(f"decode_batch-{fmt}({len(names)}x{names[0]}..,{ch}ch)", "decode_batch", ch, size, step, run, clips=names,
              calls=("glc_decode_batch" if fmt == "f32" else "glc_decode_batch_i16",))


def chunk_span(it, k):
    """Frames [f0, f0 + n) and whether chunk k of a streaming session is the last (src/codec.rs:708-717)."""
    f0 = k * CHUNK
    left = it.nf - f0
    last = left < CHUNK
    return f0, (left if last else CHUNK), last


def op_session(ch, name, what):
    it = item(ch, name)

    def step(st, mut):
        if what == "begin":
            st.sess = None
            m_prepare(st, mut, ch, name, sym("uid", ch, name))
            f0, n, _ = chunk_span(it, 0)
            got = m_d1(st, mut, 0, n * ch)
            st.sess = dict(ch=ch, name=name, next=0, fmt=None, stale=got if got[0] == "stale" else None)
            return (0,)
        fmt = "f32" if what == "next" else "i16"
        s = st.sess
        if s is None or (s["fmt"] is not None and s["fmt"] != fmt):
            return (EINVAL, 0, 0, b"", True)
        sit = item(s["ch"], s["name"])
        k = s["next"]
        f0, n, last = chunk_span(sit, k)
        stale = s["stale"]
        if s["fmt"] is None and fmt == "i16":          # the first chunk is queued again, as int16_t
            got = m_d1(st, mut, 0, n * s["ch"])
            stale = got if got[0] == "stale" else None
        if not last:
            f1, n1, _ = chunk_span(sit, k + 1)
            got = m_d1(st, mut, f1 * s["ch"], n1 * s["ch"])
            s["stale"] = got if got[0] == "stale" else None
        s["fmt"], s["next"] = fmt, k + 1
        hops = n + (1 if last else 0)
        lo, hi = f0 * HOP * s["ch"], (f0 + hops) * HOP * s["ch"]
        if last:
            st.sess = None
        return (0, hi - lo, int(last), sym("stale", stale) if stale else sym("window", s["ch"], s["name"], lo, hi, fmt), True)

    def run(env):
        L = env.g.lib
        if what == "begin":
            return done(L.glc_decode_stream_begin(env.h, env.A.streams[(ch, name, "lib")]._h))
        cap = (CHUNK + 1) * HOP * 3
        buf = host_f32(cap, 0) if what == "next" else host_i16(cap, 0)      # the pattern everywhere: nothing behind the chunk is written
        n, last = C.c_uint64(), C.c_int()
        fn = L.glc_decode_stream_next if what == "next" else L.glc_decode_stream_next_i16
        rc = fn(env.h, buf.ctypes.data, cap, C.byref(n), C.byref(last))
        if rc != 0:
            return done(rc, 0, 0, b"", host_payload(buf, 0)[1])
        # the chunk's position is the model's business: the harness cuts the part the oracle knows out of it
        return done(rc, int(n.value), int(last.value), buf[:n.value].copy(), host_payload(buf, int(n.value))[1])
    return Op(f"session-{what}" + (f"({name},{ch}ch)" if what == "begin" else ""), "session", ch, "small", step, run, clips=(name,) if what == "begin" else (),
              calls=({"begin": "glc_decode_stream_begin", "next": "glc_decode_stream_next", "next_i16": "glc_decode_stream_next_i16"}[what],))


def op_roundtrip(ch, name, how, size="small"):
    it = item(ch, name)

    def step(st, mut):
        m_forget(st, mut, "roundtrip")
        if how != "records":
            st.rt = sym("rtinfo", ch, name)
        return (0, it.n, sym("dec", ch, name, "i16" if how == "host-i16" else "f32"), True)

    def run(env):
        t, L, A = env.torch, env.g.lib, env.A
        n = C.c_uint64()
        if how == "host-f32":
            buf = host_f32(it.n)
            rc = L.glc_roundtrip(env.h, it.x.ctypes.data, PF32, 32, it.n, ch, buf.ctypes.data, PF32, it.n, C.byref(n))
            return done(rc, int(n.value), *host_payload(buf, it.n))
        if how == "host-i16":
            _, fmt, bits = INT_ITEMS[name]
            buf = host_i16(it.n)
            rc = L.glc_roundtrip(env.h, it.ints.ctypes.data, fmt, bits, it.n, ch, buf.ctypes.data, S16, it.n, C.byref(n))
            return done(rc, int(n.value), *host_payload(buf, it.n))
        out = nan_f32(t, it.n + 8)
        if how == "device":
            rc = L.glc_roundtrip_device(env.h, vp(A.x(ch, name)), it.n, ch, vp(out), it.n, C.byref(n))
        else:
            rc = L.glc_decode_device_records(env.h, vp(A.records(ch, name)), it.nf, it.n, ch, vp(out), it.n, C.byref(n))
        return lambda: (rc, int(n.value)) + payload_and_guard(out, it.n)
    return Op(f"roundtrip-{how}({name},{ch}ch)", "roundtrip", ch, size, step, run, device_only=how in ("device", "records"), clips=(name,),
              calls=({"device": "glc_roundtrip_device", "records": "glc_decode_device_records"}.get(how, "glc_roundtrip"),))


def op_roundtrip_batch(ch, names, planar, size="small", pcm=False):
    """pcm: glc_roundtrip_batch_device_pcm on the pool's integer clips, int16_t out."""
    its = [item(ch, n) for n in names]
    t_max = max(i.pc for i in its)
    shape = (len(its), ch, t_max + 3) if planar else (len(its), t_max + 3, ch)

    def step(st, mut):
        m_forget(st, mut, "roundtrip_batch")
        st.rtb = sym("rtbinfo", ch, tuple(names))
        return (0, sym("batch16" if pcm else "batch", ch, tuple(names), planar, shape))

    def run(env):
        t, g = env.torch, env.g
        keep = []
        if pcm:
            import ctx_sequence_lanes as LN
            _, fmt, bits = INT_ITEMS[names[0]]
            x, tm, lens = LN.int_batch_in(env, ch, names, planar)
            out = pat_i16(t, int(np.prod(shape))).view(shape)
        else:
            x, tm, lens, _ = batch_in(env, ch, names, planar)
            out = nan_f32(t, int(np.prod(shape))).view(shape)
        lin = layout(g, len(its), ch, planar, tm, lens, keep)
        lout = layout(g, len(its), ch, planar, tm + 3, lens, keep)
        if pcm:
            rc = g.lib.glc_roundtrip_batch_device_pcm(env.h, vp(x), fmt, bits, C.byref(lin), vp(out), S16, C.byref(lout))
        else:
            rc = g.lib.glc_roundtrip_batch_device(env.h, vp(x), C.byref(lin), vp(out), C.byref(lout))
        env.keep.append((x, keep))
        return lambda: (rc, out.cpu().numpy().tobytes())
    return Op(f"roundtrip_batch-{'pcm-' if pcm else ''}{'planar' if planar else 'interleaved'}({len(names)}x{names[0]}..,{ch}ch)", "roundtrip_batch",
              ch, size, step, run, device_only=True, clips=names,
              calls=("glc_roundtrip_batch_device_pcm" if pcm else "glc_roundtrip_batch_device",))


def status_of(ch, name, first_row=0, rows=None):
    return item(ch, name).status(first_row, rows) if name in DAMAGED else (0, 0, 0)


def m_status(st, mut, words):
    if mut == "clean_status_ored" and st.cd is not None and len(st.cd[2]) == len(words):
        words = tuple((a[0] | b[0], a[1] + b[1], a[2] or b[2]) for a, b in zip(st.cd[2], words))
    st.cd = sym("status", tuple(words))


def op_compact_decode(ch, names, batch, planar=True, size="small", fmt="f32"):
    its = [item(ch, n) for n in names]
    t_max = max(i.pc for i in its)
    shape = (len(its), ch, t_max + 3) if planar else (len(its), t_max + 3, ch)
    assert (batch or len(names) == 1) and (batch or fmt == "f32")

    def step(st, mut):
        m_forget(st, mut, "compact_decode")
        m_status(st, mut, [status_of(ch, n) for n in names])
        if not batch:
            return (0, its[0].n, sym("dec", ch, names[0], "f32"), True)
        return (0, sym("batch" if fmt == "f32" else "batch16", ch, tuple(names), planar, shape))

    def run(env):
        t, g, A = env.torch, env.g, env.A
        if not batch:
            b = A.blob(ch, names[0])
            out = nan_f32(t, its[0].n + 8)
            n = C.c_uint64()
            rc = g.lib.glc_decode_device_compact(env.h, vp(b), b.numel(), its[0].n, ch, vp(out), its[0].n, C.byref(n))
            return lambda: (rc, int(n.value)) + payload_and_guard(out, its[0].n)
        k = len(its)
        blobs = [A.blob(ch, n) for n in names]
        ptrs = (C.c_void_p * k)(*[b.data_ptr() for b in blobs])
        sizes = (C.c_uint64 * k)(*[b.numel() for b in blobs])
        ns = (C.c_uint64 * k)(*[i.n for i in its])
        out = (nan_f32 if fmt == "f32" else pat_i16)(t, int(np.prod(shape))).view(shape)
        keep = []
        lay = layout(g, k, ch, planar, t_max + 3, [i.pc for i in its], keep)
        fn = g.lib.glc_decode_batch_device_compact if fmt == "f32" else g.lib.glc_decode_batch_device_compact_i16
        rc = fn(env.h, ptrs, sizes, ns, vp(out), C.byref(lay))
        env.keep.append(keep)
        return lambda: (rc, out.cpu().numpy().tobytes())
    kind = ("batch" if batch else "one") + ("" if fmt == "f32" else "-i16")
    return Op(f"compact_decode-{kind}({'+'.join(names) if len(names) < 4 else str(len(names)) + 'x'},{ch}ch)",
              "compact_decode", ch, size, step, run, device_only=True, clips=names,
              calls=(("glc_decode_batch_device_compact" + ("" if fmt == "f32" else "_i16")) if batch else "glc_decode_device_compact",))


def crop_rows(ch, name, start, length):
    it = item(ch, name)
    p = G().plan_crop(it.n, ch, start, length)
    return p.first_frame * ch, p.n_frames * ch


def crop_status(ch, name, start, length):
    if name not in DAMAGED:
        return (0, 0, 0)
    return item(ch, name).status(*crop_rows(ch, name, start, length))


def op_crops(ch, sels, planar=True, size="small", fmt="f32"):
    """sels: (name, start, length)."""
    length = max(s[2] for s in sels)
    shape = (len(sels), ch, length + 3) if planar else (len(sels), length + 3, ch)

    def step(st, mut):
        m_forget(st, mut, "crops")
        m_status(st, mut, [crop_status(ch, *s) for s in sels])
        return (0, sym("crops" if fmt == "f32" else "crops16", ch, tuple(sels), planar, shape))

    def run(env):
        t, g, A = env.torch, env.g, env.A
        k = len(sels)
        blobs = [A.blob(ch, s[0]) for s in sels]
        ptrs = (C.c_void_p * k)(*[b.data_ptr() for b in blobs])
        sizes = (C.c_uint64 * k)(*[b.numel() for b in blobs])
        ns = (C.c_uint64 * k)(*[item(ch, s[0]).n for s in sels])
        crops = (g._lib.GlcCrop * k)(*[g._lib.GlcCrop(s[1], s[2]) for s in sels])
        out = (nan_f32 if fmt == "f32" else pat_i16)(t, int(np.prod(shape))).view(shape)
        keep = []
        lay = layout(g, k, ch, planar, length + 3, [s[2] for s in sels], keep)
        fn = g.lib.glc_decode_crops_device_compact if fmt == "f32" else g.lib.glc_decode_crops_device_compact_i16
        rc = fn(env.h, ptrs, sizes, ns, crops, vp(out), C.byref(lay))
        env.keep.append(keep)
        return lambda: (rc, out.cpu().numpy().tobytes())
    return Op(f"crops{'' if fmt == 'f32' else '-i16'}({len(sels)}x{sels[0][0]}..,{ch}ch)", "crops", ch, size, step, run, device_only=True,
              clips=[s[0] for s in sels], calls=("glc_decode_crops_device_compact" + ("" if fmt == "f32" else "_i16"),))


def op_store_encode(ch, calls, size="small", integer=False):
    """One or two glc_encode_batch_device_compact calls through one cursor (the second appends); integer: the _int twin on
    the pool's integer clips."""
    arena_bytes = sum(int(G().compact_store_bound(ch, [item(ch, n).pc for n in names])) for names in calls) + 128

    def step(st, mut):
        m_forget(st, mut, "store_encode")
        return (tuple(0 for _ in calls), sym("store", ch, tuple(tuple(c) for c in calls), arena_bytes))

    def run(env):
        t, g = env.torch, env.g
        arena = dfull(t, arena_bytes, CS.SENTINEL, np.uint8)
        cursor = dfull(t, 1, 0, np.int64)
        rcs, ents = [], []
        for names in calls:
            keep = []
            e = dfull(t, (len(names), 4), 0, np.int64)
            if integer:
                import ctx_sequence_lanes as LN
                _, fmt, bits = INT_ITEMS[names[0]]
                x, tm, lens = LN.int_batch_in(env, ch, names)
                lay = layout(g, len(names), ch, True, tm, lens, keep)
                rcs.append(g.lib.glc_encode_batch_device_compact_int(env.h, vp(x), fmt, bits, C.byref(lay), vp(arena), arena_bytes, vp(cursor), vp(e)))
            else:
                x, tm, lens, _ = batch_in(env, ch, names, True)
                lay = layout(g, len(names), ch, True, tm, lens, keep)
                rcs.append(g.lib.glc_encode_batch_device_compact(env.h, vp(x), C.byref(lay), vp(arena), arena_bytes, vp(cursor), vp(e)))
            ents.append(e)
            env.keep.append((x, keep))
        return lambda: (tuple(rcs), (tuple(e.cpu().numpy().tobytes() for e in ents), arena.cpu().numpy().tobytes(), int(cursor.item())))
    tag = f"-int({calls[0][0]}.." if integer else "("
    return Op(f"store_encode{tag}{'+'.join(str(len(c)) for c in calls)} clips,{ch}ch)", "store_encode", ch, size, step, run, device_only=True,
              clips=[n for c in calls for n in c], calls=("glc_encode_batch_device_compact" + ("_int" if integer else ""),))


def store_names(ch):
    return list(SMALL) + (["bad_header", "bad_row7"] if ch == 2 else [])


def host_store_tables(ch):
    """The host-built store of a channel count: entries and lengths of the pool's blobs laid back to back."""
    off, entries, lengths = 0, [], []
    for n in store_names(ch):
        b = item(ch, n).blob
        entries.append(S.entry(off, b.size))
        lengths.append(item(ch, n).pc)
        off += b.size + (-b.size) % 64
    return entries, lengths, off


def op_store_draw(ch, sels, length, planar=True, size="small", fmt="f32"):
    """sels: (clip index into store_names(ch), start)."""
    names = store_names(ch)
    shape = (len(sels), ch, length) if planar else (len(sels), length, ch)

    def verdicts():
        entries, lengths, ab = host_store_tables(ch)
        return [S.verdict_of(entries, lengths, ab, max(lengths), c, s, length) for c, s in sels]

    def step(st, mut):
        m_forget(st, mut, "store_draw")
        v = verdicts()
        words = [(x | S.BAD_HEADER, 0, 0) if x else crop_status(ch, names[c], s, length) for x, (c, s) in zip(v, sels)]
        m_status(st, mut, words)
        want = tuple((None, 0, length) if x else (names[c], s, length) for x, (c, s) in zip(v, sels))
        return (0, sym("crops" if fmt == "f32" else "crops16", ch, want, planar, shape))

    def run(env):
        t, g = env.torch, env.g
        arena, entries, lengths, max_len = env.A.store(ch)
        cl = t.tensor([c for c, _ in sels], dtype=t.int64).cuda()
        stt = t.tensor([s for _, s in sels], dtype=t.int64).cuda()
        out = (nan_f32 if fmt == "f32" else pat_i16)(t, int(np.prod(shape))).view(shape)
        lay = layout(g, len(sels), ch, planar, length)
        fn = g.lib.glc_decode_crops_device_store if fmt == "f32" else g.lib.glc_decode_crops_device_store_i16
        rc = fn(env.h, vp(arena), arena.numel(), vp(entries), vp(lengths), entries.shape[0], max_len, vp(cl), vp(stt), length, vp(out), C.byref(lay))
        env.keep.append((cl, stt))
        return lambda: (rc, out.cpu().numpy().tobytes())
    return Op(f"store_draw{'' if fmt == 'f32' else '-i16'}({len(sels)} crops of {length},{ch}ch)", "store_draw", ch, size, step, run, device_only=True,
              clips=[names[c] for c, _ in sels if 0 <= c < len(names)], calls=("glc_decode_crops_device_store" + ("" if fmt == "f32" else "_i16"),))


def plan_expect(assets, ch, sels, length, planar):
    g = G()
    entries, lengths, ab = host_store_tables(ch)
    arena = assets.store(ch)[0].data_ptr()
    cs, chs = (ch * length, length) if planar else (length * ch, 0)
    dirs, descs, verdicts = S.plan_model(g, arena, ab, entries, lengths, max(lengths), [c for c, _ in sels], [s for _, s in sels], length,
                                         ch, planar, cs, chs)
    return [tuple(d) for d in dirs], [[tuple(r) for r in row] for row in descs], list(verdicts)


def op_hook_r2(name, window=None):
    """glc_debug_rows_from_compact(_window) on one of the stereo blobs of crop_cases: the status words, and for the
    undamaged one the tables of compact_decode_cases.tables."""
    d = item(2, name)
    first, frames = (0, d.nf) if window is None else window
    rows = frames * 2

    def step(st, mut):
        m_forget(st, mut, "hooks")
        w = d.status(first * 2, rows)
        m_status(st, mut, [w])
        return (0, w, sym("tables", first * 2, rows) if name == "crafted" else b"")

    def run(env):
        g = env.g
        b = env.A.blob(2, name)
        rb, cnt, raw = np.zeros(rows, np.uint64), np.zeros(rows, np.uint32), np.zeros(rows, np.int64)
        stt = g._lib.GlcCompactStatus()
        if window is None:
            f = g.lib.glc_debug_rows_from_compact
            f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint16] + [C.c_void_p] * 6
            rc = f(env.h, vp(b), b.numel(), d.nf, 2, rb.ctypes.data, cnt.ctypes.data, None, raw.ctypes.data, None, C.addressof(stt))
        else:
            f = g.lib.glc_debug_rows_from_compact_window
            f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint16, C.c_uint64, C.c_uint64] + [C.c_void_p] * 6
            rc = f(env.h, vp(b), b.numel(), d.nf, 2, first, frames, rb.ctypes.data, cnt.ctypes.data, None, raw.ctypes.data, None, C.addressof(stt))
        tabs = (rb.tobytes(), cnt.tobytes(), raw.tobytes()) if name == "crafted" else b""
        return done(rc, (int(stt.flags), int(stt.n_bad_rows), int(stt.first_bad_row)), tabs)
    return Op(f"hook-rows_from_compact{'_window' if window else ''}({name})", "hooks", 2, "small", step, run, clips=(name,),
              calls=("glc_debug_rows_from_compact" + ("_window" if window else ""),))


def op_hook_store_plan(ch, sels, length, planar=True):
    def step(st, mut):
        m_forget(st, mut, "hooks")
        st.cd = None             # the planner hook clears the record and completes no decode
        return (0, sym("plan", ch, tuple(sels), length, planar))

    def run(env):
        t, g = env.torch, env.g
        f = g.lib.glc_debug_store_plan_device
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                      C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        arena, entries, lengths, max_len = env.A.store(ch)
        n = len(sels)
        hops = S.slots(length, ch)[0]
        cl = t.tensor([c for c, _ in sels], dtype=t.int64).cuda()
        stt = t.tensor([s for _, s in sels], dtype=t.int64).cuda()
        lay = layout(g, n, ch, planar, length)
        dirs, descs, verd = np.zeros(n, S.DIR_DTYPE), np.zeros(n * hops, S.DESC_DTYPE), np.zeros(n, np.uint32)
        # d_out is never written by the planner: destinations are offsets from it, and the model counts from 0
        rc = f(env.h, vp(arena), arena.numel(), vp(entries), vp(lengths), entries.shape[0], max_len, vp(cl), vp(stt), length,
               C.c_void_p(1 << 52), C.byref(lay), dirs.ctypes.data, descs.ctypes.data, verd.ctypes.data)
        return done(rc, ([tuple(d) for d in dirs.tolist()], [[tuple(r) for r in row] for row in descs.reshape(n, hops).tolist()], verd.tolist()))
    names = store_names(ch)
    return Op(f"hook-store_plan({len(sels)} crops of {length},{ch}ch)", "hooks", ch, "small", step, run,
              clips=[names[c] for c, _ in sels if 0 <= c < len(names)], calls=("glc_debug_store_plan_device",))


_pack_cases = {}


def pack_case(kind, ch):
    """The virtual record streams the pack suites already hold to their models: one per channel count."""
    key = (kind, ch)
    if key not in _pack_cases:
        if kind == "store":
            _pack_cases[key] = CS.case(f"edges-ch{ch}")
        else:
            import compact_edges as E
            name = {1: "batch-single-dense-junk", 2: "batch-one-frame-clips", 3: "batch-first-raw"}[ch]
            _pack_cases[key] = next(c for c in E._batch_cases() if c.name == name)
            assert _pack_cases[key].desc.ch == ch
    return _pack_cases[key]


def pack_expect(kind, ch):
    import compact_edges as E
    c = pack_case(kind, ch)
    if kind == "store":
        entries, blobs, cursor = CS.store_model(c.desc, c.clip_frames, c.cursor0, 1 << 40)
        img = CS.arena_image(cursor + 4096, entries, blobs)          # exactly the bytes needed are offered; 4096 more are watched
        return CS.entry_rows(entries).tobytes(), img.tobytes(), cursor
    blob, info = E.model_batch(c.desc, c.clip_frames)
    return tuple(int(v) for v in info), np.ascontiguousarray(blob, np.uint8)[:info[3]].tobytes()


def op_hook_pack(kind, ch):
    """glc_debug_compact_store_device / glc_debug_compact_batch_device on a case of compact_store_cases / compact_edges:
    they take pack_meta and the pinned table image the batch drivers use, and leave everything on the context alone."""
    def step(st, mut):
        return (0, sym("pack", kind, ch), True) if kind == "batch" else (0, sym("pack", kind, ch))

    def run(env):
        import compact_edges as E
        t, g = env.torch, env.g
        c = pack_case(kind, ch)
        clips = c.clip_frames
        d_rec = env.A.raw(("pack", kind, ch), lambda: E.materialise(c.desc).reshape(-1))
        cf_arr = (C.c_uint64 * len(clips))(*clips)
        if kind == "store":
            f = g.lib.glc_debug_compact_store_device
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint16, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
            need = pack_expect(kind, ch)[2]
            arena = dfull(t, need + 4096, CS.SENTINEL, np.uint8)
            cursor = dfull(t, 1, c.cursor0, np.int64)
            entries = dfull(t, (len(clips), 4), -1, np.int64)
            rc = f(env.h, vp(d_rec), cf_arr, len(clips), ch, vp(arena), need, vp(cursor), vp(entries))
            return lambda: (rc, (entries.cpu().numpy().tobytes(), arena.cpu().numpy().tobytes(), int(cursor.item())))
        f = g.lib.glc_debug_compact_batch_device
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint16, C.c_void_p, C.c_uint64, C.POINTER(g._lib.GlcCompactInfo)]
        cap = E.layout(ch, sum(clips), len(clips))[4]
        out = dfull(t, cap + 4096, CS.SENTINEL, np.uint8)
        info = g._lib.GlcCompactInfo()
        rc = f(env.h, vp(d_rec), cf_arr, len(clips), ch, vp(out), cap, C.byref(info))
        nb = int(info.bytes)
        a = out.cpu().numpy()
        return done(rc, ((int(info.n_frames), int(info.n_pairs), int(info.n_raw_rows), nb), a[:nb].tobytes()), bool((a[nb:] == CS.SENTINEL).all()))
    return Op(f"hook-compact_{kind}({ch}ch)", "hooks", ch, "small", step, run, device_only=kind == "store",
              calls=(f"glc_debug_compact_{kind}_device",))


def op_switch(what, value):
    def step(st, mut):
        if what == "imdct":
            if value != st.variant and mut != "variant_switch_keeps_plan":
                st.plan_uid = 0
            st.variant = value
        return (0,)

    def run(env):
        L = env.g.lib
        if what == "stream":
            if value:
                side = env.A.side_stream()
                return done(L.glc_ctx_set_stream(env.h, C.c_void_p(side.cuda_stream)))
            return done(L.glc_ctx_set_stream(env.h, None))
        f = {"imdct": L.glc_debug_set_imdct_variant, "mdct": L.glc_debug_set_mdct_variant, "screen": L.glc_debug_set_encode_screen}[what]
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int]
        return done(f(env.h, value))
    call = {"stream": "glc_ctx_set_stream", "imdct": "glc_debug_set_imdct_variant", "mdct": "glc_debug_set_mdct_variant",
            "screen": "glc_debug_set_encode_screen"}[what]
    return Op(f"switch-{what}={value}", "switch", 0, "small", step, run, calls=(call,))


def op_refused(ch, family):
    """One call of `family` that fails its argument check.  It changes what the table of DESIGN.md says it changes: a
    refused glc_decode / glc_decode_range_device closes an open session (the check comes behind that line); nothing else
    changes anything."""
    it = item(ch, "tonal9")

    def step(st, mut):
        if mut == "refused_clears_last_status":
            st.rt = st.rtb = st.cd = None
        if family in ("decode", "decode_dev") and mut != "refused_closes_nothing":
            st.sess = None
        if family in ("stream_encode", "stream_decode"):
            import ctx_sequence_lanes as LN
            LN.m_refused_push(st, mut, family, ch)
        return (EINVAL,)

    def run(env):
        t, g, A, L = env.torch, env.g, env.A, env.g.lib
        h = env.h
        n = C.c_uint64()
        if family in MOVERS + ("stream_encode", "stream_decode"):
            import ctx_sequence_lanes as LN
            return LN.run_refused(env, ch, family)
        if family == "encode":
            out = C.c_void_p()
            return done(L.glc_encode(h, it.x.ctypes.data, 512 * ch, ch, C.byref(out)))
        if family == "encode_batch":
            ptrs = (C.c_void_p * 2)(it.x.ctypes.data, it.x.ctypes.data)
            lens = (C.c_uint64 * 2)(it.n, 512 * ch)
            outs = (C.c_void_p * 2)()
            return done(L.glc_encode_batch(h, ptrs, lens, 2, ch, outs))
        if family == "encode_dev":
            out = dfull(t, int(L.glc_compact_bound(ch, it.nf)) + 8, 0, np.uint8)
            info = g._lib.GlcCompactInfo()
            return done(L.glc_compact_device_records(h, vp(A.records(ch, "tonal9")), it.nf, ch, C.c_void_p(out.data_ptr() + 4), out.numel() - 4,
                                                     C.byref(info)))
        if family == "decode":                        # cap one too small
            buf = host_f32(it.n)
            return done(L.glc_decode(h, A.streams[(ch, "tonal9", "lib")]._h, buf.ctypes.data, it.n - 1, C.byref(n)))
        if family == "decode_dev":                    # hop range out of bounds
            out = nan_f32(t, 8)
            return done(L.glc_decode_range_device(h, A.streams[(ch, "tonal9", "lib")]._h, 3, it.nf + 2, vp(out), 1 << 30))
        if family == "decode_batch":
            hs = (C.c_void_p * 2)(A.streams[(ch, "tonal9", "lib")]._h, A.streams[(ch, "one", "lib")]._h)
            offs = (C.c_uint64 * 3)()
            buf = host_f32(it.n + 513 * ch)
            return done(L.glc_decode_batch(h, hs, 2, buf.ctypes.data, it.n + 513 * ch - 1, offs))
        if family == "session":
            return done(L.glc_decode_stream_begin(h, None))
        if family == "roundtrip":
            out = nan_f32(t, it.n)
            return done(L.glc_roundtrip_device(h, vp(A.x(ch, "tonal9")), it.n, ch, vp(out), it.n - 1, C.byref(n)))
        if family == "roundtrip_batch":               # the layouts disagree in n_clips
            x, tm, lens, _ = batch_in(env, ch, ("tonal9", "one"), True)
            keep = []
            lin, lout = layout(g, 2, ch, True, tm, lens, keep), layout(g, 1, ch, True, tm, lens[:1], keep)
            out = nan_f32(t, 2 * ch * tm)
            return done(L.glc_roundtrip_batch_device(h, vp(x), C.byref(lin), vp(out), C.byref(lout)))
        if family == "compact_decode":
            b = A.blob(ch, "tonal9")
            out = nan_f32(t, it.n)
            return done(L.glc_decode_device_compact(h, vp(b), b.numel(), it.n, ch, vp(out), it.n - 1, C.byref(n)))
        if family == "crops":                         # an empty crop
            b = A.blob(ch, "tonal9")
            ptrs, sizes, ns = (C.c_void_p * 1)(b.data_ptr()), (C.c_uint64 * 1)(b.numel()), (C.c_uint64 * 1)(it.n)
            crops = (g._lib.GlcCrop * 1)(g._lib.GlcCrop(0, 0))
            out = nan_f32(t, 64)
            lay = layout(g, 1, ch, True, 0)
            return done(L.glc_decode_crops_device_compact(h, ptrs, sizes, ns, crops, vp(out), C.byref(lay)))
        if family == "store_encode":                  # an arena that is not 64-byte aligned
            x, tm, lens, _ = batch_in(env, ch, ("tonal9",), True)
            keep = []
            lay = layout(g, 1, ch, True, tm, lens, keep)
            arena = dfull(t, 1 << 20, 0, np.uint8)
            cur, e = dfull(t, 1, 0, np.int64), dfull(t, (1, 4), 0, np.int64)
            return done(L.glc_encode_batch_device_compact(h, vp(x), C.byref(lay), C.c_void_p(arena.data_ptr() + 32), (1 << 20) - 32, vp(cur), vp(e)))
        if family == "store_draw":                    # max_length < length
            arena, entries, lengths, max_len = A.store(ch)
            cl, stt = dfull(t, 1, 0, np.int64), dfull(t, 1, 0, np.int64)
            out = nan_f32(t, 600 * ch)
            lay = layout(g, 1, ch, True, 600)
            return done(L.glc_decode_crops_device_store(h, vp(arena), arena.numel(), vp(entries), vp(lengths), entries.shape[0], 599,
                                                        vp(cl), vp(stt), 600, vp(out), C.byref(lay)))
        if family == "hooks":                         # no frames
            f = L.glc_debug_rows_from_compact
            f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint16] + [C.c_void_p] * 6
            b = A.blob(2, "crafted")
            return done(f(h, vp(b), b.numel(), 0, 2, None, None, None, None, None, None))
        f = L.glc_debug_set_imdct_variant            # switch: a variant that does not exist
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int]
        return done(f(h, 7))
    return Op(f"refused-{family}({ch}ch)", "refused", ch, "small", step, run)      # its entry point is called by the family's own operations


# ------------------------------------------------------------------------------------------ the operations of a channel count

BATCH40 = tuple(SMALL[i % len(SMALL)] for i in range(40))


def crop_sels(ch, names):
    out = []
    for i, n in enumerate(names):
        pc = item(ch, n).pc
        length = min(300, pc)
        out.append((n, min(pc - length, (0, pc - length, max(0, CC.boundary_sample(1, ch) - 7))[i % 3]), length))
    return out


_ops = {}


def ops(ch):
    """name -> Op for every operation of channel count `ch`, small ones and large ones."""
    if ch in _ops:
        return _ops[ch]
    o = []
    for n in SMALL:
        o.append(op_encode(ch, n))
    o += [op_encode(ch, "tonal9_i16", "int"), op_encode(ch, "noise5_i32", "int"), op_encode(ch, "tonal9", "hooked"),
          op_encode(ch, "tonal130", size="large")]
    o += [op_encode_batch(ch, ("one", "tonal9", "noise5")), op_encode_batch(ch, ("tonal9b", "mixed13")), op_encode_batch(ch, ("tonal9_i16", "noise5_i16"), "int"),
          op_encode_batch(ch, BATCH40, size="large")]
    o += [op_encode_dev(ch, "tonal9", "range"), op_encode_dev(ch, "tonal9b", "range"), op_encode_dev(ch, "mixed13", "range"), op_encode_dev(ch, "tonal9", "mdct"),
          op_encode_dev(ch, "noise5", "compact"), op_encode_dev(ch, "tonal9", "compact"), op_encode_dev(ch, "mixed13", "frames"),
          op_encode_dev(ch, "tonal9_i16", "widen"), op_encode_dev(ch, "noise5_i32", "widen"), op_encode_dev(ch, "tonal130", "range", size="large")]
    for n in SMALL:
        o.append(op_decode(ch, n))
    o += [op_decode(ch, "tonal9", "k1"), op_decode(ch, "tonal9", "k2"), op_decode_resident(ch, "tonal9")]
    o += [op_decode(ch, "tonal9", fmt="i16"), op_decode(ch, "noise5", fmt="i16"), op_decode(ch, "tonal9b", ("as", "tonal9")),
          op_decode(ch, "tonal130", size="large")]
    o += [op_decode_device(ch, "tonal9"), op_decode_device(ch, "mixed13"), op_decode_range(ch, "tonal9", 1, 8), op_decode_range(ch, "tonal9", 1, 9),
          op_decode_range(ch, "tonal9b", 1, 8), op_decode_range(ch, "mixed13", 2, 12, "i16"), op_imdct(ch, "tonal9", 1, 9), op_imdct(ch, "tonal9", 0, 8),
          op_imdct(ch, "tonal9b", 1, 9), op_imdct(ch, "tonal130", 1, 130, size="large")]
    o += [op_decode_batch(ch, ("tonal9", "one", "noise5")), op_decode_batch(ch, ("tonal9b",)), op_decode_batch(ch, ("mixed13", "tonal9"), "i16"),
          op_decode_batch(ch, BATCH40, size="large")]
    o += [op_session(ch, "tonal9", "begin"), op_session(ch, "tonal9b", "begin"), op_session(ch, "tonal9", "next"),
          op_session(ch, "tonal9", "next_i16")]
    if ch == 1:
        o.append(op_session(1, "long1001", "begin"))
    o += [op_roundtrip(ch, "tonal9", "host-f32"), op_roundtrip(ch, "noise5", "host-f32"), op_roundtrip(ch, "tonal9_i16", "host-i16"),
          op_roundtrip(ch, "tonal9", "device"), op_roundtrip(ch, "tonal9b", "device"), op_roundtrip(ch, "noise5", "device"),
          op_roundtrip(ch, "mixed13", "device"), op_roundtrip(ch, "tonal9", "records"), op_roundtrip(ch, "noise5", "records"),
          op_roundtrip(ch, "tonal130", "device", size="large")]
    o += [op_roundtrip_batch(ch, ("tonal9", "one", "mixed13"), True), op_roundtrip_batch(ch, ("tonal9b", "one"), False),
          op_roundtrip_batch(ch, ("noise5", "noise5"), True), op_roundtrip_batch(ch, ("tonal9", "tonal9b"), True),
          op_roundtrip_batch(ch, BATCH40, False, size="large")]
    o += [op_compact_decode(ch, ("tonal9",), False), op_compact_decode(ch, ("tonal9b",), False), op_compact_decode(ch, ("noise5",), False),
          op_compact_decode(ch, ("mixed13", "one", "tonal9"), True), op_compact_decode(ch, ("tonal9b", "noise5"), True, planar=False),
          op_compact_decode(ch, BATCH40, True, size="large"), op_compact_decode(ch, ("tonal130",), False, size="large")]
    o += [op_crops(ch, crop_sels(ch, ("tonal9", "mixed13", "noise5", "one"))), op_crops(ch, crop_sels(ch, ("tonal9b", "tonal9")), planar=False),
          op_crops(ch, crop_sels(ch, ("noise5", "tonal9b", "tonal9b"))),
          op_crops(ch, crop_sels(ch, BATCH40), size="large")]
    o += [op_store_encode(ch, [("tonal9", "one", "noise5")]), op_store_encode(ch, [("tonal9b", "one")]), op_store_encode(ch, [("mixed13", "tonal9b"), ("one", "tonal9")]),
          op_store_encode(ch, [BATCH40], size="large")]
    o += [op_store_draw(ch, [(1, 0), (4, 100), (3, 17), (0, 0), (2, 9000)], 300), op_store_draw(ch, [(2, 5), (2, 9016)], 200), op_store_draw(ch, [(2, 5), (1, 5), (7, 0), (1, -1)], 400, planar=False),
          op_store_draw(ch, [(i % 5, 3 * i) for i in range(40)], 300, size="large")]
    o += [op_hook_pack("store", ch), op_hook_pack("batch", ch), op_hook_r2("crafted"), op_hook_r2("crafted", (2, 3)),
          op_hook_store_plan(ch, [(1, 0), (2, 5), (3, 40), (9, 0)], 300), op_hook_store_plan(ch, [(2, 0), (2, 7)], 200),
          op_encode_dev(ch, "tonal9", "quantize")]
    # dealt in this order by the walk: every change is taken back by the operation that follows it
    o += [op_switch("imdct", 5), op_switch("imdct", 0), op_switch("mdct", 1), op_switch("mdct", 0), op_switch("screen", 2), op_switch("screen", 0),
          op_switch("stream", 1), op_switch("stream", 0), op_switch("imdct", 1)]
    o += [op_refused(ch, f) for f in FAMILIES if f != "refused"]
    # the newer entry points of the older families, and the five newer families
    import ctx_sequence_lanes as LN
    o += [op_store_encode(ch, [("tonal9_i16", "noise5_i16")], integer=True), op_store_encode(ch, [("noise5_i32", "tonal9_i32")], integer=True),
          op_roundtrip_batch(ch, ("tonal9_i16", "noise5_i16"), True, pcm=True),
          op_compact_decode(ch, ("tonal9", "one", "noise5"), True, fmt="i16"), op_compact_decode(ch, ("tonal9b", "mixed13"), True, planar=False, fmt="i16"),
          op_crops(ch, crop_sels(ch, ("tonal9", "noise5", "one")), fmt="i16"), op_crops(ch, crop_sels(ch, ("tonal9b", "mixed13")), planar=False, fmt="i16"),
          op_store_draw(ch, [(1, 0), (4, 100), (3, 17), (9, 0)], 300, fmt="i16"), op_store_draw(ch, [(2, 5), (2, 9016)], 200, planar=False, fmt="i16")]
    o += LN.ops(ch)
    if ch == 2:                  # the damaged blobs: dirty calls, and the clean ones that follow them
        o += [op_compact_decode(2, ("bad_header",), False), op_compact_decode(2, ("bad_row7",), False), op_compact_decode(2, ("crafted",), False),
              op_compact_decode(2, ("bad_row7", "bad_header", "crafted"), True),
              op_crops(2, [("bad_header", 1280, 2048), ("bad_row7", 1280, 2048), ("crafted", 1280, 2048)]),
              op_store_draw(2, [(5, 1280), (6, 1280), (1, 0)], 2048), op_hook_r2("bad_header"), op_hook_r2("bad_row7"),
              op_hook_r2("bad_row7", (2, 3)), op_hook_r2("bad_header", (2, 3))]
    _ops[ch] = {op.name: op for op in o}
    assert len(_ops[ch]) == len(o), "operation names must be unique"
    return _ops[ch]


def by_family(ch, family, size="small"):
    return [op for op in ops(ch).values() if op.family == family and op.size == size]


# ------------------------------------------------------------------------------------------ sequences

def _pick(ch, fam, k=0, **kw):
    c = by_family(ch, fam, **kw)
    return c[k % len(c)]


def euler_walk(rng):
    """A closed walk over the 21 families that takes every ordered pair (self pairs included) exactly once: 442 vertices."""
    n = len(FAMILIES)
    out_edges = {a: list(range(n)) for a in range(n)}
    for a in out_edges:
        rng.shuffle(out_edges[a])
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if out_edges[v]:
            stack.append(out_edges[v].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == n * n + 1
    return [FAMILIES[i] for i in walk]


def generated(seed=20261019):
    """The seeded part: the Euler walk, cut into one piece per channel count (the cut operation repeated, so that no
    pair is lost); the operation of a family is dealt round-robin, a session operation by what the model says is open."""
    rng = random.Random(seed)
    walk = euler_walk(rng)
    third = len(walk) // 3
    pieces = {1: walk[:third + 1], 2: walk[third:2 * third + 1], 3: walk[2 * third:]}
    seqs = []
    for ch, fams in pieces.items():
        st, used, seq = State(), {}, []
        for f in fams:
            if f == "session":
                if st.sess is None:
                    op = ops(ch)[f"session-begin({'long1001' if ch == 1 else 'tonal9'},{ch}ch)"]
                else:
                    op = ops(ch)["session-next" if used.get("n", 0) % 3 != 2 else "session-next_i16"]
                    used["n"] = used.get("n", 0) + 1
            else:
                op = _pick(ch, f, used.get(f, 0))
                used[f] = used.get(f, 0) + 1
            op.step(st, None)
            seq.append(op)
        seqs.append((f"walk-{ch}ch", seq))
    return seqs


def directed():
    seqs = []
    for ch in CHS:
        o = ops(ch)
        dA, dB, dBig = o[f"decode-f32(tonal9/lib,{ch}ch)"], o[f"decode-f32(tonal9b/lib,{ch}ch)"], o[f"decode-f32(tonal130/lib,{ch}ch)"]
        k1, k2, res = o[f"decode-f32(tonal9/k1,{ch}ch)"], o[f"decode-f32(tonal9/k2,{ch}ch)"], o[f"decode_resident(tonal9,{ch}ch)"]
        v = {n: o[f"switch-imdct={n}"] for n in (0, 1, 5)}
        # 3: the plan cache
        plan = [dA, dA, dB, dA, o[f"decode_range-f32(tonal9,1..8,{ch}ch)"], dA, o[f"decode_range-f32(tonal9,1..9,{ch}ch)"], dA,
                o[f"imdct_device+overlap_add(tonal9,1..9,{ch}ch)"], dA, o[f"imdct_device+overlap_add(tonal9,0..8,{ch}ch)"], dA,
                o[f"imdct_device+overlap_add(tonal9,1..9,{ch}ch)"], o[f"imdct_device+overlap_add(tonal9,0..8,{ch}ch)"],
                o[f"decode_range-f32(tonal9,1..9,{ch}ch)"], dA, v[5], dA, v[0], dA, v[1], dA, v[0], dA, dBig, dA,
                k1, o[f"decode-f32(tonal9b/id-of-tonal9,{ch}ch)"], k1, k2, res]
        seqs.append((f"plan-cache-{ch}ch", plan))
        # 2: sandwiches, the operation of X on tonal9 where it has one and on tonal9b
        sand = []
        for f in FAMILIES:
            cands = by_family(ch, f)
            same = next((c for c in cands if "tonal9" in c.clips), cands[0])
            other = next((c for c in cands if "tonal9b" in c.clips and "tonal9" not in c.clips), None)
            xs = [same] + ([o[f"hook-compact_store({ch}ch)"], o[f"hook-compact_batch({ch}ch)"]] if f == "hooks" else [])
            for x in xs:
                for after in (dA, res, k2) if ch == 2 else (res,):
                    sand += [k1, x, after]
            if ch == 2 and other is not None:     # switch and refused work on no clip
                sand += [k1, other, res, k1, other, k2, k1, other, dA]
        seqs.append((f"sandwiches-{ch}ch", sand))
        # 4: sessions
        name = "long1001" if ch == 1 else "tonal9"
        begin, nxt, nxt16 = o[f"session-begin({name},{ch}ch)"], o["session-next"], o["session-next_i16"]
        sess = []
        for f in FAMILIES:
            if f == "session":
                sess += [begin, nxt, o[f"session-begin(tonal9b,{ch}ch)"], nxt]
            else:
                sess += [begin, nxt, _pick(ch, f, 1), nxt]
        for x in (o[f"hook-compact_store({ch}ch)"], o[f"hook-compact_batch({ch}ch)"]):
            sess += [begin, nxt, x, nxt]
        # the session goes on on a caller's stream, and back on the context's own
        sess += [begin, nxt, o["switch-stream=1"], nxt, o["switch-stream=0"], nxt, begin, o["switch-stream=1"], nxt, nxt, o["switch-stream=0"], nxt]
        sess += [begin, nxt, nxt16, nxt, nxt, begin, nxt16, nxt, nxt16]          # formats do not mix
        sess += [begin, nxt, o[f"refused-decode({ch}ch)"], nxt, begin, nxt, o[f"refused-decode_dev({ch}ch)"], nxt]    # these two close it
        if ch == 1:              # the only stream of more than one chunk is mono
            seqs.append((f"sessions-{ch}ch", sess))
        # 5: small, large, small
        order = []
        for f in FAMILIES:
            big = by_family(ch, f, size="large")
            if big:
                s = _pick(ch, f, 0)
                order += [s, big[0], s]
        seqs.append((f"size-order-{ch}ch", order))
        # 6: raw counters in front of a tonal round trip
        seqs.append((f"raw-before-tonal-{ch}ch", [o[f"roundtrip-device(noise5,{ch}ch)"], o[f"roundtrip-device(tonal9,{ch}ch)"],
                                                  o[f"roundtrip-host-f32(noise5,{ch}ch)"], o[f"roundtrip-host-f32(tonal9,{ch}ch)"],
                                                  o[f"roundtrip_batch-planar(2xnoise5..,{ch}ch)"], o[f"roundtrip_batch-planar(2xtonal9..,{ch}ch)"]]))
        # the records are there when the calls that must leave them alone run: RT, RTB and CD, then
        # glc_decode_device_records, every refused call, the pack hooks, and the same on a caller's stream
        keepers = [o[f"roundtrip-records(noise5,{ch}ch)"], o[f"roundtrip-records(tonal9,{ch}ch)"]] + \
                  [o[f"refused-{f}({ch}ch)"] for f in FAMILIES if f != "refused"] + [_pick(ch, f, ch) for f in MOVERS] + \
                  [o[f"hook-compact_store({ch}ch)"], o[f"hook-compact_batch({ch}ch)"], o[f"decode-i16(tonal9/lib,{ch}ch)"]]
        have = [o[f"roundtrip-device(mixed13,{ch}ch)"], o[f"roundtrip_batch-planar(3xtonal9..,{ch}ch)"],
                o["compact_decode-batch(bad_row7+bad_header+crafted,2ch)"] if ch == 2 else o[f"compact_decode-batch(mixed13+one+tonal9,{ch}ch)"]]
        seqs.append((f"records-kept-{ch}ch", have + keepers + [o["switch-stream=1"]] + have + keepers[:4] + [dA, o["switch-stream=0"], dA, res]))
        # device-only calls of the newer families back to back: a mover directly behind a draw (whose planner has the device
        # write rtb_tab), a crops / batch call directly behind a mover (the uploaded image again), pushes on both kinds of
        # lane that complete frames, an eviction, and the _i16 and ragged draws between them
        e0, d0 = o[f"stream_enc-dev-il(lane0:tonal9,{ch}ch)"], o[f"stream_dec-dev-f32(lane0:tonal9,{ch}ch)"]
        draw = o[f"store_draw(5 crops of 300,{ch}ch)"]
        seqs.append((f"queued-movers-{ch}ch", [
            draw, o[f"store_join(tonal9@3/7,{ch}ch)"], o[f"crops(4xtonal9..,{ch}ch)"], o[f"store_cut-split(A,{ch}ch)"],
            o[f"roundtrip_batch-planar(3xtonal9..,{ch}ch)"], o[f"store_compact-in_place(A:0111,{ch}ch)"], draw, o[f"store_cut-trim(B,{ch}ch)"],
            e0, e0, d0, e0, d0, d0, o[f"stream_enc-dev-s16(lane0:tonal9_i16,{ch}ch)"], o[f"stream_dec-dev-i16(lane1:tonal9b,{ch}ch)"],
            o[f"store_ragged-f32(6 crops of 600,{ch}ch)"], o[f"store_join(tonal9b@2/5,{ch}ch)"], o[f"crops-i16(3xtonal9..,{ch}ch)"],
            o[f"store_compact-copy_out(A:1011,{ch}ch)"], o[f"store_ragged-i16(3 crops of 600,{ch}ch)"], o[f"stream_dec-empty({ch}ch)"], e0, d0]))
        # a refused push moves no lane: the push behind it takes the next chunk
        seqs.append((f"lane-rules-{ch}ch", [e0, e0, o[f"refused-stream_encode({ch}ch)"], e0, d0, o[f"refused-stream_decode({ch}ch)"], d0,
                                            o[f"stream_dec-empty({ch}ch)"], d0, e0]))
        # every lane operation through its whole plan - the chunk that completes nothing, the one that ends on a completion
        # point, the finish - and once more, which starts the clip over; an encoder lane and a decoder lane take turns
        enc = [op for op in by_family(ch, "stream_encode")]
        dec = [op for op in by_family(ch, "stream_decode") if op.lane and op.lane[1][0] == ch and "whole" not in op.name]
        whole = []
        for j, e in enumerate(enc):
            d = dec[j % len(dec)]
            for r in range(6):
                whole += [e] + ([d] if r < 4 else [])
        seqs.append((f"lane-plans-{ch}ch", whole))
    seqs.append(("lane-interrupts", lane_interrupts()))
    o = ops(2)
    seqs.append(("dirty-before-clean", [
        o["compact_decode-one(bad_header,2ch)"], o["compact_decode-one(crafted,2ch)"], o["compact_decode-one(bad_row7,2ch)"], o["compact_decode-one(tonal9,2ch)"],
        o["compact_decode-batch(bad_row7+bad_header+crafted,2ch)"], o["compact_decode-batch(mixed13+one+tonal9,2ch)"],
        o["crops(3xbad_header..,2ch)"], o["crops(3xbad_header..,2ch)"], o["crops(4xtonal9..,2ch)"],
        o["store_draw(3 crops of 2048,2ch)"], o["store_draw(5 crops of 300,2ch)"],
        o["hook-rows_from_compact(bad_header)"], o["hook-rows_from_compact(crafted)"], o["hook-rows_from_compact(bad_row7)"], o["hook-rows_from_compact(crafted)"],
        o["hook-rows_from_compact_window(bad_row7)"], o["hook-rows_from_compact_window(crafted)"],
        o["hook-rows_from_compact_window(bad_header)"], o["hook-rows_from_compact_window(crafted)"],
        o["compact_decode-one(bad_header,2ch)"], o["refused-compact_decode(2ch)"], o["hook-store_plan(4 crops of 300,2ch)"],
        # a push whose segment is a damaged blob, a clean one, a damaged one again, and a push without segments: CD is
        # dirty, clean, dirty and empty
        o["stream_dec-whole(lane1:bad_row7,2ch)"], o["stream_dec-whole(lane1:crafted,2ch)"], o["stream_dec-whole(lane1:bad_row7,2ch)"],
        o["stream_dec-empty(2ch)"], o["stream_dec-whole(lane1:bad_row7,2ch)"], o["store_cut-split(A,2ch)"], o["refused-stream_decode(2ch)"]]))
    return seqs


def is_mid_clip(ln):
    """A lane that holds samples back (encoder) or a carry (decoder): something taken, the clip not finished."""
    return ln is not None and not ln["finished"] and ln["at"] > 0


def lane_interrupts():
    """For every family X the runs "push, X, push" on an encoder lane and on a decoder lane in mid-clip, host and device
    lanes and the channel counts in turn.  The pushes are dealt by the model: a lane is pushed until it is in mid-clip, X
    runs, and the next push completes frames from what the lane held."""
    st, seq = State(), []

    def push(op):
        op.step(st, None)
        seq.append(op)

    for i, f in enumerate(FAMILIES):
        ch = CHS[i % len(CHS)]
        o = ops(ch)
        how = ("dev-il", "dev") if i % 2 else ("host", "host")
        for a in (o[f"stream_enc-{how[0]}(lane0:tonal9,{ch}ch)"], o[f"stream_dec-{how[1]}-f32(lane0:tonal9,{ch}ch)"]):
            kind, key = a.lane
            lanes = st.enc if kind == "enc" else st.dec
            push(a)
            while not is_mid_clip(lanes.get(key)):
                push(a)
            cands = by_family(ch, f)
            x = next(c for c in cands[i % len(cands):] + cands if c.lane != a.lane)
            push(x)
            push(a)
    return seq


_seqs = None


def sequences():
    global _seqs
    if _seqs is None:
        _seqs = generated() + directed()
        _seqs += the_rest(_seqs)
    return _seqs


def the_rest(seqs):
    """Every operation that no sequence above has drawn, per channel count, in a seeded order behind a context that
    holds a resident stream and all three records: no operation runs on fresh contexts only."""
    used = {op.name for _, s in seqs for op in s}
    out = []
    for ch in CHS:
        o = ops(ch)
        rest = [op for op in o.values() if op.name not in used]
        used |= {op.name for op in rest}
        random.Random(7 + ch).shuffle(rest)
        if rest:
            head = [o[f"roundtrip-device(tonal9,{ch}ch)"], o[f"roundtrip_batch-planar(3xtonal9..,{ch}ch)"],
                    o[f"compact_decode-one(tonal9,{ch}ch)"], o[f"decode-f32(tonal9/k1,{ch}ch)"]]
            out.append((f"the-rest-{ch}ch", head + rest + [o["switch-stream=0"], o["switch-imdct=0"], o[f"decode-f32(tonal9/lib,{ch}ch)"]]))
    return out


# The number of the first queued run of the sequences the 16-family suite had, when the runs were numbered through all
# sequences.  The runs are numbered per sequence now, from these numbers on (from 0 for a newer sequence), so that a test id
# keeps naming the same run of the same sequence whatever sequences are added around it.
QUEUED_FIRST = {"walk-1ch": 0, "walk-2ch": 4, "walk-3ch": 8, "plan-cache-1ch": 13, "size-order-1ch": 14, "records-kept-1ch": 17,
                "plan-cache-2ch": 19, "size-order-2ch": 20, "records-kept-2ch": 23, "plan-cache-3ch": 25, "size-order-3ch": 26,
                "records-kept-3ch": 29, "dirty-before-clean": 31, "the-rest-1ch": 32, "the-rest-2ch": 33, "the-rest-3ch": 35}


def queued_sequences():
    """For every sequence its longest runs of operations that only queue (device entry points that do not synchronise),
    named "<sequence>@<number>" (QUEUED_FIRST)."""
    out = []
    for name, seq in sequences():
        run, k = [], QUEUED_FIRST.get(name, 0)
        for op in list(seq) + [None]:
            if op is not None and op.device_only:
                run.append(op)
                continue
            if len(run) >= 3:
                out.append((f"{name}@{k}", run))
                k += 1
            run = []
    assert len({n for n, _ in out}) == len(out)
    return out


# ------------------------------------------------------------------------------------------ entry-point coverage

def _exempt(reason, *names):
    return {n: reason for n in names}


# Every function include/glc.h exports is called by an operation that runs in a sequence (Op.calls), or is here with the
# reason why no operation needs to call it.  tests/test_ctx_sequences.py fails on a name that is on neither side.
EXEMPT = {
    **_exempt("makes or destroys the context the harness runs every sequence on", "glc_ctx_create", "glc_ctx_destroy"),
    **_exempt("called by the harness behind every operation", "glc_ctx_synchronize", "glc_roundtrip_last_info", "glc_roundtrip_batch_last_info",
              "glc_decode_compact_last_status", "glc_ctx_resident_stream"),
    **_exempt("a getter: reads the context or a session and writes nothing", "glc_last_error", "glc_ctx_stream", "glc_ctx_device", "glc_ctx_tables",
              "glc_stream_dec_frames_done", "glc_stream_enc_max_push", "glc_stream_dec_max_push", "glc_version"),
    **_exempt("records two events on the context's stream and touches nothing the table lists", "glc_ctx_timer_begin", "glc_ctx_timer_end"),
    **_exempt("host only, takes no context: a planner or a size", "glc_plan_encode", "glc_record_bytes", "glc_compact_bound", "glc_plan_crop",
              "glc_compact_store_bound", "glc_store_crop_slots", "glc_store_ragged_slots", "glc_plan_stream_push", "glc_plan_stream_dec_push"),
    **_exempt("host only, takes no context: a twin the expected values are made with", "glc_compact_records", "glc_frames_to_compact",
              "glc_compact_join", "glc_compact_cut", "glc_frames_from_compact", "glc_frames_from_records"),
    **_exempt("host only, takes no context: works on a glc_frames object", "glc_decoded_len", "glc_serialized_size", "glc_serialize", "glc_deserialize",
              "glc_save", "glc_load", "glc_frames_free", "glc_frames_info", "glc_frame_is_raw", "glc_frame_sparse", "glc_frame_scale", "glc_frame_raw",
              "glc_frames_get_view", "glc_frames_from_parts", "glc_frames_from_gather", "glc_frames_stream_id"),
    **_exempt("host only, takes no context: audio files", "glc_wav_load", "glc_wav_save16", "glc_free", "glc_flac_encode", "glc_flac_save",
              "glc_flac_load", "glc_flac_decode", "glc_audio_load_pcm", "glc_wav_save16_i16", "glc_flac_encode_i16", "glc_flac_save_i16"),
}


def exported(header):
    """The function names a header declares: an identifier glc_... directly in front of "(" at the start of a declaration."""
    import re
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return set(re.findall(r"^[A-Za-z_][\w \*]*?\b(glc_\w+)\s*\(", text, flags=re.M))


def model_run(seq, mut=None):
    """The modelled results of a sequence on a fresh context: per operation its outputs + the tail."""
    st = State()
    res = []
    for op in seq:
        res.append(tuple(op.step(st, mut)) + st.tail())
    return res
