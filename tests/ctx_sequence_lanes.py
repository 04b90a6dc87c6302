"""Builders for tests/ctx_sequence_cases.py: the five newer call families of DESIGN.md section 4 ("What a call leaves on
its context") - store_compact, store_join, store_cut, stream_encode, stream_decode - and the newer entry points of the
older ones (ragged draws, the _int store encode, the _i16 store and crop decodes).  A plain module; nothing here touches
the GPU until an operation's `run` is called.

Expected values come from outside the code under test, and from models that exist already: segment blobs from the host
twin of the packing on the oracle's range records (what glc_encode_range_device + glc_compact_device_records give),
joined and cut blobs from glc_compact_join / glc_compact_cut held to the models of store_join_cases / store_cut_cases,
evictions from store_compact_cases.compact, ragged verdicts from store_ragged_cases, push plans from
stream_encode_cases.model_plan / stream_decode_cases.model_plan, PCM from the CPU oracle.

The lanes.  A context under test holds at most one open stream encoder and one open stream decoder per channel count and
push kind (a session takes host pushes or device pushes, never both - include/glc.h), two lanes each, opened by the first
operation that needs them.  A lane operation is bound to a lane and a clip and is dealt by the model: where the model says
the lane holds that clip unfinished it pushes the next chunk of the clip's fixed plan, otherwise it resets the lane and
starts the clip over.  `step` leaves its decision in State.pending and `run` carries it out, so the library is never asked
what a lane holds.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

import compact_store_cases as CS
import crop_cases as CC
import ctx_sequence_cases as Q
import roundtrip_cases as RC
import store_compact_cases as SC
import store_cut_cases as SCUT
import store_join_cases as J
import store_ragged_cases as RG
import stream_decode_cases as SD
import stream_encode_cases as SE
from ctx_sequence_cases import EINVAL, F32, HOP, I16_PATTERN, NAN_BITS, PF32, S16, S32, Op, item, sym

MOVERS = ("store_compact", "store_join", "store_cut")
PATTERN = SC.PATTERN
MARGIN = 256
N_LANES = 2
spent = [0.0]                     # seconds of expected-value work done here: tests hold it to the pool's budget


def timed(fn):
    def wrapper(*a, **kw):
        t0 = time.perf_counter()
        try:
            return fn(*a, **kw)
        finally:
            spent[0] += time.perf_counter() - t0
    return wrapper


# ------------------------------------------------------------------------------------------ blobs of frame ranges

_segs = {}


@timed
def seg_blob(ch, name, f0, n):
    """The blob of frames [f0, f0 + n) of a pool clip: the packing's host twin on those of the oracle's range records."""
    key = (ch, name, f0, n)
    if key not in _segs:
        it = item(ch, name)
        rec = it.records.reshape(it.nf, -1)[f0:f0 + n]
        _segs[key] = np.ascontiguousarray(Q.G().compact_records(np.ascontiguousarray(rec).reshape(-1), ch), np.uint8)
    return _segs[key]


def row5(blob, off):
    p, r, nb = Q.blob_counts(blob)
    assert nb == blob.size and nb % 64 == 0
    return [off, blob.size, p, r, 1]


def lay_out(blobs):
    """(arena image, rows [offset, bytes, n_pairs, n_raw_rows, stored]) of blobs back to back."""
    rows, off = [], 0
    for b in blobs:
        rows.append(row5(b, off))
        off += b.size
    return (np.concatenate(blobs) if blobs else np.zeros(0, np.uint8)), rows


def ranges(nf, bounds):
    edges = [0] + list(bounds) + [nf]
    return [(a, b - a) for a, b in zip(edges, edges[1:])]


STORES = {"A": ("tonal9", "noise5", "tonal9b", "mixed13"), "B": ("tonal9b", "one", "mixed13"), "big": ("tonal130",)}

_stores = {}


@timed
def mover_store(ch, which):
    """A store built on the host from the twins' blobs: (arena image, rows of 5, lengths)."""
    key = (ch, which)
    if key not in _stores:
        arena, rows = lay_out([item(ch, n).blob_enc for n in STORES[which]])
        _stores[key] = (arena, rows, [item(ch, n).pc for n in STORES[which]])
    return _stores[key]


def padded(a, margin=MARGIN):
    return np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.full(margin, PATTERN, np.uint8)])


def up(env, a):
    return env.torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pat(env, nbytes):
    return up(env, np.full(nbytes, PATTERN, np.uint8))


def host(t):
    return t.cpu().numpy().tobytes()


def m_mover(st, mut, family):
    """The rule of the three movers: nothing on the context changes."""
    if mut == f"{family}_forgets":
        st.plan_of = ("other", family)
        st.sess, st.res_id, st.plan_uid = None, 0, 0
    if mut == "mover_clears_last_status":
        st.cd = None


# ------------------------------------------------------------------------------------------ store_compact

@timed
def evict_expect(ch, which, keep, in_place):
    arena, rows, lengths = mover_store(ch, which)
    entries = [SC.entry(o, b, p, r, s) for o, b, p, r, s in rows]
    dst = None if in_place else np.full(arena.size + 128, PATTERN, np.uint8)
    w = SC.compact(arena, arena.size, entries, lengths, list(keep), dst, None if in_place else dst.size)
    n = len(rows)
    return (padded(w["arena"]).tobytes(), padded(np.array(w["entries"], np.uint64).reshape(n, 4)).tobytes(),
            padded(np.array(w["lengths"], np.int64)).tobytes(), padded(np.array(w["new_index"], np.int64)).tobytes(),
            padded(np.array([w["n_out"], w["cursor"]], np.uint64)).tobytes())


def op_store_compact(ch, which, keep, in_place, rnd=0, size="small"):
    keep = tuple(keep)

    def step(st, mut):
        m_mover(st, mut, "store_compact")
        return (0, 0, 0, sym("evict", ch, which, keep, in_place))

    def run(env):
        L = env.g.lib
        arena_h, rows, lengths = mover_store(ch, which)
        n, ab = len(rows), arena_h.size
        arena = up(env, padded(arena_h))
        dst = arena if in_place else pat(env, ab + 128 + MARGIN)
        ent = up(env, J.entry_words(rows))
        lens = up(env, np.array(lengths, np.int64))
        kp = up(env, np.array(keep, np.uint8))
        outs = [pat(env, k * n + MARGIN) for k in (32, 8, 8)] + [pat(env, 16 + MARGIN)]
        rc0 = L.glc_debug_set_store_compact_round(env.h, rnd) if rnd else 0      # the switch, and back behind the call
        rc = L.glc_store_compact_device(env.h, arena.data_ptr(), ab, ent.data_ptr(), lens.data_ptr(), n, kp.data_ptr(), dst.data_ptr(),
                                        ab if in_place else ab + 128, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                        outs[3].data_ptr(), outs[3].data_ptr() + 8)
        rc1 = L.glc_debug_set_store_compact_round(env.h, 0) if rnd else 0
        env.keep.append((arena, dst, ent, lens, kp, outs))
        return lambda: (rc0, rc, rc1, (host(dst),) + tuple(host(o) for o in outs))
    tag = "".join(str(k) for k in keep)
    return Op(f"store_compact-{'in_place' if in_place else 'copy_out'}({which}:{tag}{',round=' + str(rnd) if rnd else ''},{ch}ch)", "store_compact",
              ch, size, step, run, device_only=True, clips=STORES[which],
              calls=("glc_store_compact_device",) + (("glc_debug_set_store_compact_round",) if rnd else ()))


# ------------------------------------------------------------------------------------------ store_join

@timed
def join_expect(ch, name, bounds, dst_bytes, cursor):
    it = item(ch, name)
    blobs = [seg_blob(ch, name, f0, n) for f0, n in ranges(it.nf, bounds)]
    arena, rows = lay_out(blobs)
    segs = [(0, f0, n) for f0, n in ranges(it.nf, bounds)]
    w = J.join_store(arena, arena.size, rows, segs, [it.pc], ch, np.full(dst_bytes, PATTERN, np.uint8), dst_bytes, cursor)
    at, nb = w["entries"][0][:2]
    joined = w["dst"][at:at + nb].tobytes()
    twin = Q.G().compact_join([b.tobytes() for b in blobs], ch)
    assert joined == bytes(twin) == it.blob_enc.tobytes(), "the model, glc_compact_join and the whole clip's blob are one"
    return (padded(w["dst"]).tobytes(), padded(J.entry_words(w["entries"])).tobytes(), padded(np.array(w["lengths"], np.int64)).tobytes(),
            padded(np.array(w["status"], np.uint32)).tobytes(), padded(np.array([w["cursor"]], np.uint64)).tobytes())


def untouched(*sizes):
    return tuple(np.full(s + MARGIN, PATTERN, np.uint8).tobytes() for s in sizes)


def op_store_join(ch, name, bounds, size="small", empty=False):
    it = item(ch, name)
    bounds = tuple(bounds)
    cursor = 100

    def dst_bytes():
        return 128 + it.blob_enc.size + 192

    def step(st, mut):
        m_mover(st, mut, "store_join")
        return (0, sym("nojoin", ch, name, len(bounds) + 1) if empty else sym("join", ch, name, bounds))

    def run(env):
        g, L = env.g, env.g.lib
        rs = ranges(it.nf, bounds)
        arena = env.A.raw(("segarena", ch, name, bounds), lambda: lay_out([seg_blob(ch, name, f0, n) for f0, n in rs])[0])
        ent = env.A.raw(("segentries", ch, name, bounds), lambda: J.entry_words(lay_out([seg_blob(ch, name, f0, n) for f0, n in rs])[1]))
        dst = pat(env, dst_bytes() + MARGIN)
        outs = [pat(env, 32 + MARGIN), pat(env, 8 + MARGIN), pat(env, 4 * len(rs) + MARGIN)]
        cur = up(env, padded(np.array([cursor], np.uint64)))
        segs = (g._lib.GlcStreamSeg * len(rs))(*[g._lib.GlcStreamSeg(0, f0, n) for f0, n in rs])
        lens = (C.c_uint64 * 1)(it.pc)
        rc = L.glc_store_join_segments_device(env.h, arena.data_ptr(), arena.numel(), ent.data_ptr(), segs, 0 if empty else len(rs), lens, ch,
                                              dst.data_ptr(), dst_bytes(), cur.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                              outs[2].data_ptr())
        env.keep.append((dst, outs, cur, segs, lens))
        return lambda: (rc, (host(dst), host(outs[0]), host(outs[1]), host(outs[2]), host(cur)))
    return Op(f"store_join({name}@{'none' if empty else '/'.join(map(str, bounds))},{ch}ch)", "store_join", ch, size, step, run, device_only=True,
              clips=(name,), calls=("glc_store_join_segments_device",))


# ------------------------------------------------------------------------------------------ store_cut

@timed
def cut_expect(ch, which, cuts, dst_bytes, cursor):
    arena, rows, _ = mover_store(ch, which)
    w = SCUT.cut_store(arena, arena.size, rows, list(cuts), None, ch, np.full(dst_bytes, PATTERN, np.uint8), dst_bytes, cursor)
    assert not any(w["status"])
    for (clip, f0, n), e in zip(cuts, w["entries"]):
        twin = Q.G().compact_cut(item(ch, STORES[which][clip]).blob_enc.tobytes(), f0, n, ch)
        assert w["dst"][e[0]:e[0] + e[1]].tobytes() == bytes(twin) == seg_blob(ch, STORES[which][clip], f0, n).tobytes(), \
            "the model, glc_compact_cut and the blob of the frame range are one"
    return (padded(w["dst"]).tobytes(), padded(J.entry_words(w["entries"])).tobytes(), padded(np.array(w["lengths"], np.int64)).tobytes(),
            padded(np.array(w["status"], np.uint32)).tobytes(), padded(np.array([w["cursor"]], np.uint64)).tobytes())


def op_store_cut(ch, which, cuts, tag, size="small"):
    cuts = tuple(cuts)
    cursor = 100
    k = max(len(cuts), 1)

    def dst_bytes():
        return 128 + sum(seg_blob(ch, STORES[which][c], f0, n).size for c, f0, n in cuts) + 192

    def step(st, mut):
        m_mover(st, mut, "store_cut")
        return (0, sym("cut", ch, which, cuts) if cuts else sym("nocut",))

    def run(env):
        g, L = env.g, env.g.lib
        arena = env.A.raw(("moverarena", ch, which), lambda: mover_store(ch, which)[0])
        ent = env.A.raw(("moverentries", ch, which), lambda: J.entry_words(mover_store(ch, which)[1]))
        dst = pat(env, dst_bytes() + MARGIN)
        outs = [pat(env, 32 * k + MARGIN), pat(env, 8 * k + MARGIN), pat(env, 4 * k + MARGIN)]
        cur = up(env, padded(np.array([cursor], np.uint64)))
        arr = (g._lib.GlcStoreCut * k)(*[g._lib.GlcStoreCut(*c) for c in cuts])
        rc = L.glc_store_cut_device(env.h, arena.data_ptr(), arena.numel(), ent.data_ptr(), ent.shape[0], arr, len(cuts), None, ch,
                                    dst.data_ptr(), dst_bytes(), cur.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())
        env.keep.append((dst, outs, cur, arr))
        return lambda: (rc, (host(dst), host(outs[0]), host(outs[1]), host(outs[2]), host(cur)))
    return Op(f"store_cut-{tag}({which},{ch}ch)", "store_cut", ch, size, step, run, device_only=True,
              clips=tuple(STORES[which][c] for c, _, _ in cuts) or STORES[which][:1], calls=("glc_store_cut_device",))


# ------------------------------------------------------------------------------------------ the lanes

def enc_plan(pc):
    """The fixed chunk plan of a clip, in samples per channel: a chunk that completes no frame, one that ends exactly on the
    completion point of frame 0 (1536), two that end between completion points, and the rest with the finish."""
    head = [1000, 536, 3000, 2500]
    assert SE.frames_done(1000) == 0 and SE.frames_done(1535) == 0 and SE.frames_done(1536) == 1 and pc > sum(head) + 512
    return head + [pc - sum(head)]


def dec_plan(nf):
    """The fixed push plan of a clip, in frames per segment: one segment, two segments, the rest with the finish."""
    assert nf >= 9
    return [(3,), (2, 2), (nf - 7,)]


def offsets(plan):
    out = [0]
    for p in plan:
        out.append(out[-1] + (sum(p) if isinstance(p, tuple) else p))
    return out


def lane_decision(lanes, key, name, plan):
    """(lane record, restart, index of the push in the plan or None where the lane is somewhere no plan leads)."""
    ln = lanes.get(key)
    restart = ln is None or ln["name"] != name or ln["finished"]
    if restart:
        ln = dict(name=name, at=0, finished=False, segs=())
    offs = offsets(plan)[:-1]
    return ln, restart, (offs.index(ln["at"]) if ln["at"] in offs else None)


def frames_of(L, ch=1):
    return RC.frames_of(L)


def session(env, kind, ch, cls):
    """The context's one open stream encoder / decoder of a channel count and push kind, opened on first use."""
    key = (kind, ch, cls)
    if key not in env.sessions:
        s = C.c_void_p()
        fn = env.g.lib.glc_stream_enc_open if kind == "enc" else env.g.lib.glc_stream_dec_open
        assert fn(env.h, ch, N_LANES, C.byref(s)) == 0
        env.sessions[key] = s
    return env.sessions[key]


def close_sessions(env):
    for (kind, _, _), s in env.sessions.items():
        (env.g.lib.glc_stream_enc_close if kind == "enc" else env.g.lib.glc_stream_dec_close)(s)
    env.sessions.clear()


def per_lane(ctype, lane, value):
    a = (ctype * N_LANES)()
    a[lane] = value
    return a


# ------------------------------------------------------------------------------------------ stream_encode

@timed
def segstore_expect(ch, name, f0, n, arena_bytes):
    """(entry rows, arena image, cursor) of a device push into a fresh arena: one segment at 0, or nothing at all."""
    rows = np.zeros((N_LANES, 4), np.int64)
    if n == 0:
        return rows.tobytes(), np.full(arena_bytes, CS.SENTINEL, np.uint8).tobytes(), 0
    b = seg_blob(ch, name, f0, n)
    entries, bl, cursor = CS.store_model(None, None, 0, arena_bytes, blobs=[(b,) + Q.blob_counts(b)[:2]])
    rows[:1] = CS.entry_rows(entries)
    return rows.tobytes(), CS.arena_image(arena_bytes, entries, bl).tobytes(), cursor


def op_stream_encode(ch, name, lane, how):
    """how: "host" (glc_stream_enc_push, float), "dev-il" (device push, interleaved float), "dev-s16" (device push, planar
    int16_t; the clip is one of the pool's integer clips)."""
    it = item(ch, name)
    cls = "host" if how == "host" else "dev"
    key = (ch, cls, lane)
    plan = enc_plan(it.pc)

    def arena_bytes():
        return int(Q.G().compact_store_bound(ch, [it.pc])) + 128

    def step(st, mut):
        ln, restart, k = lane_decision(st.enc, key, name, plan)
        Q.m_forget(st, mut, "stream_encode")
        if k is None:
            st.pending = None
            return (0, sym("stale", ("lane", key, ln["at"])))
        finish = k == len(plan) - 1
        f0, n, _ = SE.model_plan(ln["at"], plan[k], finish, frames_of)
        segs = ln["segs"] + (((f0, n),) if n else ())
        st.pending = dict(restart=restart, at=ln["at"], n_new=plan[k], finish=finish)
        st.enc[key] = dict(name=name, at=ln["at"] + plan[k], finished=finish, segs=segs)
        if cls == "host":
            return (0, segs, sym("segs", ch, name, segs), sym("glc", ch, name) if finish else b"")
        return (0, ((lane, f0, n),) if n else (), sym("segstore", ch, name, f0, n, arena_bytes()))

    def run(env):
        g, L, t = env.g, env.g.lib, env.torch
        p = env.st.pending
        s = session(env, "enc", ch, cls)
        if p["restart"]:
            assert L.glc_stream_enc_reset(s, lane) == 0
        n, at = p["n_new"], p["at"]
        fin = per_lane(C.c_uint8, lane, int(p["finish"]))
        if cls == "host":
            chunk = np.ascontiguousarray(it.x[at * ch:(at + n) * ch])
            rc = L.glc_stream_enc_push(s, per_lane(C.c_void_p, lane, chunk.ctypes.data), PF32, 32, per_lane(C.c_uint64, lane, chunk.size),
                                       C.cast(fin, C.c_void_p))
            k = C.c_uint64()
            assert L.glc_stream_enc_segments(s, lane, C.byref(k)) == 0
            got, blobs = [], []
            for j in range(k.value):
                ptr, nb, f0, nf = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64()
                assert L.glc_stream_enc_segment(s, lane, j, C.byref(ptr), C.byref(nb), C.byref(f0), C.byref(nf)) == 0
                got.append((f0.value, nf.value))
                blobs.append(C.string_at(ptr.value, nb.value))
            whole = b""
            if p["finish"] and rc == 0:
                out = C.c_void_p()
                assert L.glc_stream_enc_frames(s, lane, C.byref(out)) == 0
                whole = Q.frames_to_bytes(env, out.value)
            return Q.done(rc, tuple(got), tuple(blobs), whole)
        planar = how == "dev-s16"
        src = (it.ints if planar else it.x).reshape(-1, ch)[at:at + n]
        shape = (N_LANES, ch, n) if planar else (N_LANES, n, ch)
        if planar:
            words = Q.fill_batch(shape, True, [src if i == lane else src[:0] for i in range(N_LANES)], ch, np.int16, -32768)
            x = t.from_numpy(words).cuda()
        else:
            x = t.from_numpy(Q.fill_batch(shape, False, [src if i == lane else src[:0] for i in range(N_LANES)], ch).view(F32)).cuda()
        keep = []
        lay = Q.layout(g, N_LANES, ch, planar, n, [n if i == lane else 0 for i in range(N_LANES)], keep)
        ab = arena_bytes()
        arena = Q.dfull(t, ab, CS.SENTINEL, np.uint8)
        cursor, ent = Q.dfull(t, 1, 0, np.int64), Q.dfull(t, (N_LANES, 4), 0, np.int64)
        segs = (g._lib.GlcStreamSeg * N_LANES)()
        n_segs = C.c_uint64()
        rc = L.glc_stream_enc_push_device(s, Q.vp(x), S16 if planar else PF32, 16 if planar else 32, C.byref(lay), C.cast(fin, C.c_void_p),
                                          Q.vp(arena), ab, Q.vp(cursor), Q.vp(ent), segs, C.byref(n_segs))
        got = tuple((int(q.stream), int(q.first_frame), int(q.n_frames)) for q in segs[:n_segs.value])
        env.keep.append((x, keep, fin))
        return lambda: (rc, got, (host(ent), host(arena), int(cursor.item())))
    calls = ("glc_stream_enc_open", "glc_stream_enc_close", "glc_stream_enc_reset") + \
        (("glc_stream_enc_push", "glc_stream_enc_segments", "glc_stream_enc_segment", "glc_stream_enc_frames") if cls == "host"
         else ("glc_stream_enc_push_device",))
    op = Op(f"stream_enc-{how}(lane{lane}:{name},{ch}ch)", "stream_encode", ch, "small", step, run, device_only=cls == "dev", clips=(name,),
            calls=calls)
    op.lane = ("enc", key)
    return op


# ------------------------------------------------------------------------------------------ stream_decode

def span(it, s0, s1, fmt):
    d = it.dec if fmt == "f32" else it.dec16
    return d[s0 * it.ch:s1 * it.ch]


def lanes_out(ch, name, lane, s0, s1, fmt, planar, shape):
    arrays = [span(item(ch, name), s0, s1, fmt) if i == lane else np.zeros(0, F32 if fmt == "f32" else np.int16) for i in range(N_LANES)]
    if fmt == "f32":
        return Q.fill_batch(shape, planar, arrays, ch).tobytes()
    return Q.fill_batch(shape, planar, arrays, ch, np.int16, I16_PATTERN).tobytes()


def dec_segments(ch, name):
    it = item(ch, name)
    return [(f0, n) for f0, n in ranges(it.nf, offsets([q for p in dec_plan(it.nf) for q in p])[1:-1])]


def push_out(env, ch, lane, n, fmt, planar):
    """(the output tensor of a device push in which `lane` emits n samples per channel, its layout, what to keep alive)."""
    t = env.torch
    T = n + 3
    shape = (N_LANES, ch, T) if planar else (N_LANES, T, ch)
    size = int(np.prod(shape))
    out = (Q.nan_f32(t, size) if fmt == "f32" else Q.pat_i16(t, size)).view(shape)
    keep = []
    lay = Q.layout(env.g, N_LANES, ch, planar, T, [n if i == lane else 0 for i in range(N_LANES)], keep)
    lay.length = 0
    return out, lay, keep, shape


def op_stream_decode(ch, name, lane, how, fmt):
    """how: "host" (glc_stream_dec_push) or "dev" (glc_stream_dec_push_device; f32 interleaved, S16 planar)."""
    it = item(ch, name)
    key = (ch, how, lane)
    plan = dec_plan(it.nf)
    planar = fmt == "i16"

    def step(st, mut):
        ln, restart, k = lane_decision(st.dec, key, name, plan)
        Q.m_forget(st, mut, "stream_decode")
        if k is None:
            st.pending = None
            return (0, sym("stale", ("lane", key, ln["at"])))
        finish = k == len(plan) - 1
        n = sum(plan[k])
        s0, ns = SD.model_plan(ln["at"], n, finish, it.pc)
        if mut != "stream_decode_leaves_last_status":
            Q.m_status(st, mut, [(0, 0, 0)] * len(plan[k]))
        st.pending = dict(restart=restart, k=k, finish=finish, n=ns)
        st.dec[key] = dict(name=name, at=ln["at"] + n, finished=finish, segs=())
        if how == "host":
            return (0, tuple(ns * ch if i == lane else 0 for i in range(N_LANES)), sym("span", ch, name, s0, s0 + ns, fmt), True)
        shape = (N_LANES, ch, ns + 3) if planar else (N_LANES, ns + 3, ch)
        return (0, sym("lanes_out", ch, name, lane, s0, s0 + ns, fmt, planar, shape))

    def run(env):
        g, L = env.g, env.g.lib
        p = env.st.pending
        s = session(env, "dec", ch, how)
        if p["restart"]:
            assert L.glc_stream_dec_reset(s, lane) == 0
        first = sum(len(q) for q in plan[:p["k"]])
        mine = dec_segments(ch, name)[first:first + len(plan[p["k"]])]
        segs = (g._lib.GlcStreamSeg * len(mine))(*[g._lib.GlcStreamSeg(lane, f0, n) for f0, n in mine])
        fin = per_lane(C.c_uint8, lane, int(p["finish"]))
        tot = per_lane(C.c_uint64, lane, it.pc if p["finish"] else 0)
        if how == "host":
            blobs = [seg_blob(ch, name, f0, n) for f0, n in mine]
            ptrs = (C.c_void_p * len(mine))(*[b.ctypes.data for b in blobs])
            sizes = (C.c_uint64 * len(mine))(*[b.size for b in blobs])
            buf = Q.host_f32(p["n"] * ch) if fmt == "f32" else Q.host_i16(p["n"] * ch)
            n_out = (C.c_uint64 * N_LANES)()
            rc = L.glc_stream_dec_push(s, ptrs, sizes, segs, len(mine), C.cast(fin, C.c_void_p), tot, per_lane(C.c_void_p, lane, buf.ctypes.data),
                                       PF32 if fmt == "f32" else S16, n_out)
            return Q.done(rc, tuple(int(v) for v in n_out), *Q.host_payload(buf, p["n"] * ch))
        all_segs = dec_segments(ch, name)
        arena = env.A.raw(("decarena", ch, name), lambda: lay_out([seg_blob(ch, name, f0, n) for f0, n in all_segs])[0])
        ent = env.A.raw(("decentries", ch, name), lambda: J.entry_words(lay_out([seg_blob(ch, name, f0, n) for f0, n in all_segs])[1]))
        out, lay, keep, _ = push_out(env, ch, lane, p["n"], fmt, planar)
        rc = L.glc_stream_dec_push_device(s, Q.vp(arena), arena.numel(), C.c_void_p(ent.data_ptr() + 32 * first), segs, len(mine),
                                          C.cast(fin, C.c_void_p), tot, Q.vp(out), PF32 if fmt == "f32" else S16, C.byref(lay))
        env.keep.append((keep, segs, fin, tot))
        return lambda: (rc, host(out))
    calls = ("glc_stream_dec_open", "glc_stream_dec_close", "glc_stream_dec_reset", "glc_stream_dec_push" if how == "host" else "glc_stream_dec_push_device")
    op = Op(f"stream_dec-{how}-{fmt}(lane{lane}:{name},{ch}ch)", "stream_decode", ch, "small", step, run, device_only=how == "dev", clips=(name,),
            calls=calls)
    op.lane = ("dec", key)
    return op


def op_stream_decode_empty(ch):
    """A device push without segments and without a finish: accepted, it emits nothing, moves no lane and leaves CD empty."""
    def step(st, mut):
        Q.m_forget(st, mut, "stream_decode")
        if mut != "empty_push_keeps_last_status" and mut != "stream_decode_leaves_last_status":
            st.cd = None
        return (0, True)

    def run(env):
        L = env.g.lib
        s = session(env, "dec", ch, "dev")
        arena = env.A.raw(("decarena", ch, "tonal9"), lambda: lay_out([seg_blob(ch, "tonal9", f0, n) for f0, n in dec_segments(ch, "tonal9")])[0])
        out = Q.nan_f32(env.torch, 64)
        keep = []
        lay = Q.layout(env.g, N_LANES, ch, False, 8, [0] * N_LANES, keep)
        lay.length = 0
        rc = L.glc_stream_dec_push_device(s, Q.vp(arena), arena.numel(), None, None, 0, None, None, Q.vp(out), PF32, C.byref(lay))
        env.keep.append(keep)
        return lambda: (rc, Q.payload_and_guard(out, 0)[1])
    return Op(f"stream_dec-empty({ch}ch)", "stream_decode", ch, "small", step, run, device_only=True,
              calls=("glc_stream_dec_open", "glc_stream_dec_close", "glc_stream_dec_push_device"))


def op_stream_decode_whole(name, lane=1):
    """A stereo blob of crop_cases / compact_decode_cases, damaged or not, as the one segment of a whole stream: the lane is
    reset, takes the blob with the finish, and CD holds the segment's words."""
    d = item(2, name)
    key = (2, "dev", lane)

    def step(st, mut):
        Q.m_forget(st, mut, "stream_decode")
        if mut != "stream_decode_leaves_last_status":
            Q.m_status(st, mut, [d.status()])
        st.dec[key] = dict(name=name, at=d.nf, finished=True, segs=())
        return (0, sym("lanes_out", 2, name, lane, 0, d.pc, "f32", False, (N_LANES, d.pc + 3, 2)))

    def run(env):
        g, L = env.g, env.g.lib
        s = session(env, "dec", 2, "dev")
        assert L.glc_stream_dec_reset(s, lane) == 0
        b = env.A.blob(2, name)
        ent = env.A.raw(("wholeentry", name), lambda: J.entry_words([[0, d.blob.size, 0, 0, 1]]))
        segs = (g._lib.GlcStreamSeg * 1)(g._lib.GlcStreamSeg(lane, 0, d.nf))
        fin, tot = per_lane(C.c_uint8, lane, 1), per_lane(C.c_uint64, lane, d.pc)
        out, lay, keep, _ = push_out(env, 2, lane, d.pc, "f32", False)
        rc = L.glc_stream_dec_push_device(s, Q.vp(b), b.numel(), Q.vp(ent), segs, 1, C.cast(fin, C.c_void_p), tot, Q.vp(out), PF32, C.byref(lay))
        env.keep.append((keep, segs, fin, tot))
        return lambda: (rc, host(out))
    op = Op(f"stream_dec-whole(lane{lane}:{name},2ch)", "stream_decode", 2, "small", step, run, device_only=True, clips=(name,),
            calls=("glc_stream_dec_open", "glc_stream_dec_close", "glc_stream_dec_reset", "glc_stream_dec_push_device"))
    op.lane = ("dec", key)
    return op


# ------------------------------------------------------------------------------------------ the refusals of the five

def m_refused_push(st, mut, family, ch):
    """A refused push changes nothing, the lanes included."""
    if mut == "refused_push_moves_lane":
        lanes = st.enc if family == "stream_encode" else st.dec
        key = (ch, "dev", 0)
        if key in lanes:
            lanes[key] = dict(lanes[key], at=lanes[key]["at"] + 1)


def run_refused(env, ch, family):
    g, t, L, A = env.g, env.torch, env.g.lib, env.A
    if family == "store_compact":                     # an arena that is not 64-byte aligned
        arena_h, rows, lengths = mover_store(ch, "B")
        n = len(rows)
        arena, ent = up(env, padded(arena_h)), up(env, J.entry_words(rows))
        kp, outs = up(env, np.ones(n, np.uint8)), [pat(env, 32 * n), pat(env, 8 * n), pat(env, 16)]
        return Q.done(L.glc_store_compact_device(env.h, arena.data_ptr() + 32, arena_h.size - 64, ent.data_ptr(), None, n, kp.data_ptr(),
                                                 arena.data_ptr() + 32, arena_h.size - 64, outs[0].data_ptr(), None, outs[1].data_ptr(),
                                                 outs[2].data_ptr(), outs[2].data_ptr() + 8))
    if family == "store_join":                        # a clip whose first segment does not start at frame 0
        arena, ent = up(env, seg_blob(ch, "tonal9", 0, 3)), up(env, J.entry_words([row5(seg_blob(ch, "tonal9", 0, 3), 0)]))
        segs = (g._lib.GlcStreamSeg * 1)(g._lib.GlcStreamSeg(0, 1, 3))
        dst, outs, cur = pat(env, 1 << 16), [pat(env, 32), pat(env, 8)], up(env, np.zeros(1, np.uint64))
        return Q.done(L.glc_store_join_segments_device(env.h, arena.data_ptr(), arena.numel(), ent.data_ptr(), segs, 1, None, ch, dst.data_ptr(),
                                                       1 << 16, cur.data_ptr(), outs[0].data_ptr(), None, outs[1].data_ptr()))
    if family == "store_cut":                         # a cut of no frames
        arena_h, rows, _ = mover_store(ch, "B")
        arena, ent = up(env, arena_h), up(env, J.entry_words(rows))
        cuts = (g._lib.GlcStoreCut * 1)(g._lib.GlcStoreCut(0, 2, 0))
        dst, outs, cur = pat(env, 1 << 16), [pat(env, 32), pat(env, 8), pat(env, 8)], up(env, np.zeros(1, np.uint64))
        return Q.done(L.glc_store_cut_device(env.h, arena.data_ptr(), arena.numel(), ent.data_ptr(), len(rows), cuts, 1, None, ch, dst.data_ptr(),
                                             1 << 16, cur.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr()))
    if family == "stream_encode":                     # a layout of one clip for a session of two lanes
        s = session(env, "enc", ch, "dev")
        x = Q.nan_f32(t, 64 * ch)
        lay = Q.layout(g, 1, ch, False, 64)
        arena, cursor, ent = Q.dfull(t, 1 << 16, 0, np.uint8), Q.dfull(t, 1, 0, np.int64), Q.dfull(t, (N_LANES, 4), 0, np.int64)
        segs, n_segs = (g._lib.GlcStreamSeg * N_LANES)(), C.c_uint64()
        return Q.done(L.glc_stream_enc_push_device(s, Q.vp(x), PF32, 32, C.byref(lay), None, Q.vp(arena), 1 << 16, Q.vp(cursor), Q.vp(ent), segs,
                                                   C.byref(n_segs)))
    s = session(env, "dec", ch, "dev")                # stream_decode: a segment that is not at its lane's frames done
    b = up(env, seg_blob(ch, "tonal9", 0, 3))
    ent = up(env, J.entry_words([row5(seg_blob(ch, "tonal9", 0, 3), 0)]))
    segs = (g._lib.GlcStreamSeg * 1)(g._lib.GlcStreamSeg(0, 1 << 20, 3))
    out = Q.nan_f32(t, N_LANES * 3 * HOP * ch)
    keep = []
    lay = Q.layout(g, N_LANES, ch, False, 3 * HOP, [3 * HOP, 0], keep)
    lay.length = 0
    return Q.done(L.glc_stream_dec_push_device(s, Q.vp(b), b.numel(), Q.vp(ent), segs, 1, None, None, Q.vp(out), PF32, C.byref(lay)))


REFUSED_CALLS = {"store_compact": ("glc_store_compact_device",), "store_join": ("glc_store_join_segments_device",),
                 "store_cut": ("glc_store_cut_device",), "stream_encode": ("glc_stream_enc_push_device",),
                 "stream_decode": ("glc_stream_dec_push_device",)}


# ------------------------------------------------------------------------------------------ the newer calls of older families

def ragged_rows(ch, sels, length):
    """Per selection (clip name or None, start, valid length) and its status words, by store_ragged_cases' rule."""
    names = Q.store_names(ch)
    entries, lengths, ab = Q.host_store_tables(ch)
    rows, words = [], []
    for c, s, w in sels:
        v = RG.verdict_of(entries, lengths, ab, max(lengths), c, s, w, length)
        if v:
            rows.append((None, 0, 0))
            words.append((v | RG.BAD_HEADER, 0, 0))
        else:
            valid = RG.valid_of(lengths[c], s, w, length)
            rows.append((names[c], s, valid))
            words.append(Q.crop_status(ch, names[c], s, valid))
    return rows, words


def ragged_out(ch, rows, length, fmt, shape):
    """A pattern tensor (n, ch, T) with every row's `length` samples per channel written: the valid part, then zeros."""
    dt, patt = (np.uint32, NAN_BITS) if fmt == "f32" else (np.int16, I16_PATTERN)
    want = np.full(shape, patt, dt)
    want[:, :, :length] = 0
    for i, (n, s, v) in enumerate(rows):
        if n is not None:
            d = item(ch, n).dec if fmt == "f32" else item(ch, n).dec16
            want[i, :, :v] = np.ascontiguousarray(d).view(dt).reshape(-1, ch)[s:s + v].T
    return want.tobytes()


def op_store_ragged(ch, sels, length, fmt="f32", size="small"):
    """sels: (clip index into store_names(ch), start, wanted length or None)."""
    names = Q.store_names(ch)
    sels = tuple(sels)
    shape = (len(sels), ch, length + 3)

    def step(st, mut):
        Q.m_forget(st, mut, "store_draw")
        rows, words = ragged_rows(ch, sels, length)
        Q.m_status(st, mut, words)
        return (0, sym("ragged", ch, sels, length, fmt, shape), tuple(v for _, _, v in rows))

    def run(env):
        t, g = env.torch, env.g
        arena, entries, lengths, max_len = env.A.store(ch)
        i64 = lambda v: t.tensor(list(v), dtype=t.int64).cuda()
        cl, stt, want = i64(c for c, _, _ in sels), i64(s for _, s, _ in sels), i64(length if w is None else w for _, _, w in sels)
        valid = Q.dfull(t, len(sels), -7, np.int64)
        size_ = int(np.prod(shape))
        out = (Q.nan_f32(t, size_) if fmt == "f32" else Q.pat_i16(t, size_)).view(shape)
        keep = []
        lay = Q.layout(g, len(sels), ch, True, length + 3, [length] * len(sels), keep)
        fn = g.lib.glc_decode_ragged_crops_device_store if fmt == "f32" else g.lib.glc_decode_ragged_crops_device_store_i16
        rc = fn(env.h, Q.vp(arena), arena.numel(), Q.vp(entries), Q.vp(lengths), entries.shape[0], max_len, Q.vp(cl), Q.vp(stt), Q.vp(want), length,
                Q.vp(out), C.byref(lay), Q.vp(valid))
        env.keep.append((cl, stt, want, keep))
        return lambda: (rc, host(out), tuple(valid.cpu().tolist()))
    return Op(f"store_ragged-{fmt}({len(sels)} crops of {length},{ch}ch)", "store_draw", ch, size, step, run, device_only=True,
              clips=[names[c] for c, _, _ in sels if 0 <= c < len(names)],
              calls=("glc_decode_ragged_crops_device_store" + ("" if fmt == "f32" else "_i16"),))


def batch16(ch, names, planar, shape):
    return Q.fill_batch(shape, planar, [item(ch, n).dec16 for n in names], ch, np.int16, I16_PATTERN).tobytes()


def crops16(ch, sels, planar, shape):
    """crop_cases.want_crops for int16_t outputs: (name or None, start, length) per crop."""
    want = np.full(shape, I16_PATTERN, np.int16)
    for i, (n, s, l) in enumerate(sels):
        piece = item(ch, n).dec16.reshape(-1, ch)[s:s + l] if n else np.zeros((l, ch), np.int16)
        assert piece.shape[0] == l
        if planar:
            want[i, :ch, :l] = piece.T
        else:
            want[i, :l, :ch] = piece
    return want.tobytes()


def int_batch_in(env, ch, names, planar=True):
    """The integer clips of a batch in a (B, C, T) device tensor of their sample type, a loud value behind every clip."""
    its = [item(ch, n) for n in names]
    t = max(i.pc for i in its)
    dt = its[0].ints.dtype
    x = Q.fill_batch((len(its), ch, t) if planar else (len(its), t, ch), planar, [i.ints for i in its], ch, dt, 12345)
    return env.torch.from_numpy(x).cuda(), t, [i.pc for i in its]


# ------------------------------------------------------------------------------------------ bytes of the symbols made here

def materialise(v, assets=None):
    kind = v[1]
    if kind == "evict":
        return evict_expect(*v[2:])
    if kind == "join":
        _, _, ch, name, bounds = v
        return join_expect(ch, name, bounds, 128 + item(ch, name).blob_enc.size + 192, 100)
    if kind == "nojoin":
        _, _, ch, name, n_segs = v
        return untouched(128 + item(ch, name).blob_enc.size + 192, 32, 8, 4 * n_segs) + (padded(np.array([100], np.uint64)).tobytes(),)
    if kind == "cut":
        _, _, ch, which, cuts = v
        return cut_expect(ch, which, cuts, 128 + sum(seg_blob(ch, STORES[which][c], f0, n).size for c, f0, n in cuts) + 192, 100)
    if kind == "nocut":
        return untouched(128 + 192, 32, 8, 4) + (padded(np.array([100], np.uint64)).tobytes(),)
    if kind == "segs":
        _, _, ch, name, segs = v
        return tuple(seg_blob(ch, name, f0, n).tobytes() for f0, n in segs)
    if kind == "segstore":
        return segstore_expect(*v[2:])
    if kind == "span":
        _, _, ch, name, s0, s1, fmt = v
        return span(item(ch, name), s0, s1, fmt).tobytes()
    if kind == "lanes_out":
        return lanes_out(*v[2:])
    if kind == "ragged":
        _, _, ch, sels, length, fmt, shape = v
        return ragged_out(ch, ragged_rows(ch, sels, length)[0], length, fmt, shape)
    if kind == "batch16":
        return batch16(*v[2:])
    if kind == "crops16":
        return crops16(*v[2:])
    raise KeyError(f"no bytes for {v}")


# ------------------------------------------------------------------------------------------ the operations of a channel count

JOIN_BOUNDS = {"tonal9": (3, 7), "tonal9b": (2, 5), "mixed13": (2, 6, 9), "tonal130": (40, 90)}


def ops(ch):
    o = [op_store_compact(ch, "A", (0, 1, 1, 1), True), op_store_compact(ch, "A", (1, 0, 1, 1), False), op_store_compact(ch, "A", (0, 0, 0, 0), True),
         op_store_compact(ch, "A", (1, 1, 1, 1), False), op_store_compact(ch, "B", (0, 1, 1), False), op_store_compact(ch, "B", (1, 0, 1), True),
         op_store_compact(ch, "A", (0, 1, 1, 1), True, rnd=4096, size="large")]
    o += [op_store_join(ch, n, JOIN_BOUNDS[n]) for n in ("tonal9", "tonal9b", "mixed13")]
    o += [op_store_join(ch, "tonal9", JOIN_BOUNDS["tonal9"], empty=True), op_store_join(ch, "tonal130", JOIN_BOUNDS["tonal130"], size="large")]
    o += [op_store_cut(ch, "A", ((0, 0, 3), (0, 3, 4), (0, 7, 2)), "split"), op_store_cut(ch, "B", ((0, 1, 7),), "trim"),
          op_store_cut(ch, "A", ((3, 0, 13), (3, 5, 4), (1, 0, 5)), "resend"), op_store_cut(ch, "B", (), "none"),
          op_store_cut(ch, "big", ((0, 0, 50), (0, 50, 80), (0, 10, 100)), "split", size="large")]
    o += [op_stream_encode(ch, "tonal9", 0, "dev-il"), op_stream_encode(ch, "tonal9b", 1, "dev-il"), op_stream_encode(ch, "tonal9", 0, "host"),
          op_stream_encode(ch, "tonal9b", 1, "host"), op_stream_encode(ch, "tonal9_i16", 0, "dev-s16"), op_stream_encode(ch, "mixed13", 1, "dev-il")]
    o += [op_stream_decode(ch, "tonal9", 0, "dev", "f32"), op_stream_decode(ch, "tonal9b", 1, "dev", "i16"), op_stream_decode(ch, "tonal9", 0, "host", "f32"),
          op_stream_decode(ch, "tonal9b", 1, "host", "i16"), op_stream_decode(ch, "mixed13", 1, "dev", "f32"), op_stream_decode_empty(ch)]
    o += [op_store_ragged(ch, [(0, 0, None), (0, 100, 300), (1, 9000, None), (3, 17, 1), (9, 0, None), (2, 0, 0)], 600),
          op_store_ragged(ch, [(0, 13, None), (4, 13000, None), (2, 5, 200)], 600, "i16")]
    if ch == 2:
        o += [op_stream_decode_whole("bad_row7"), op_stream_decode_whole("crafted")]
    return o
