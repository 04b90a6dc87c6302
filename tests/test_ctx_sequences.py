"""One long-lived context against fresh ones, across every family of entry points ("What a call leaves
on its context").

The same operations (tests/ctx_sequence_cases.py) run on ONE context that lives through a long, mixed sequence and must
give, bit for bit, what the CPU oracle, the host twins and the suite's models say each call gives alone: outputs over the
whole buffer (a NaN payload where nothing may be written), return codes, and after every call the three "last call"
getters and glc_ctx_resident_stream as the model of the context's bookkeeping predicts them.

The CPU tests hold the sequences to the coverage conditions (every ordered pair of families adjacent, sandwiches, the plan
cache patterns, interrupted sessions, interrupted encoder and decoder lanes, small-large-small, dirty before clean, the
queued runs of the device-only calls, every exported entry point called or exempt) and show that every modelled slip of
the bookkeeping changes a modelled result (the power test).  Where the oracle cannot know a sample - the 512 positions in
front of the gapless trim and the padding behind it, in the un-trimmed outputs of glc_decode_device and the streaming
chunks - the comparison covers the known part and the pattern behind the buffer.
"""
import ctypes as C
import time

import numpy as np
import pytest

import ctx_sequence_cases as Q

EINVAL = Q.EINVAL
gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ CPU: the sequences

def all_ops():
    return [op for _, seq in Q.sequences() for op in seq]


def windows(k):
    for name, seq in Q.sequences():
        for i in range(len(seq) - k + 1):
            yield name, seq[i:i + k]


def test_the_pool_is_what_its_names_say():
    t0 = time.perf_counter()
    for ch in Q.CHS:
        raw = {n: [f["raw"] is not None for f in Q.item(ch, n).parsed["frames"]] for n in Q.SMALL + ("tonal130",)}
        assert [len(raw[n]) for n in Q.SMALL] == [1, 9, 9, 5, 13] and len(raw["tonal130"]) == 130
        assert not any(raw["tonal9"]) and not any(raw["tonal9b"]) and not any(raw["tonal130"]) and all(raw["noise5"])
        assert any(raw["mixed13"]) and not all(raw["mixed13"])
        a, b = Q.item(ch, "tonal9"), Q.item(ch, "tonal9b")
        assert a.n == b.n and a.glc != b.glc and a.info[2] != b.info[2]          # same shape, other content and pair count
        for n in ("tonal9_i16", "noise5_i32"):
            assert Q.item(ch, n).dec.size == Q.item(ch, n).n
        assert Q.item(ch, "tonal9").dec16.dtype == np.int16
    assert len(Q.item(1, "long1001").parsed["frames"]) == 1001 > 2 * Q.CHUNK
    for n in ("bad_header", "bad_row7", "crafted"):
        assert Q.item(2, n).dec.size == Q.item(2, n).n
    assert not Q.item(2, "bad_header").dec.view(np.uint32).any()
    assert time.perf_counter() - t0 < 45.0, "the oracle work of the pool must stay well under a minute"


def test_every_expected_value_has_bytes():
    """Every element of every modelled result of the unmutated model resolves from the pool (ids and planner records
    need the device assets; a "stale" symbol would mean the model itself predicts a wrong decode)."""
    seen = set()
    for name, seq in Q.sequences():
        for op, res in zip(seq, Q.model_run(seq)):
            for v in res:
                if Q.is_sym(v) and v not in seen:
                    seen.add(v)
                    assert v[1] != "stale", (name, op, v)
                    if v[1] not in ("uid", "plan"):
                        assert Q.materialise(v) is not None


def test_adjacency_every_ordered_pair_of_families():
    have = {(s[0].family, s[1].family) for _, s in windows(2)}
    missing = [(a, b) for a in Q.FAMILIES for b in Q.FAMILIES if (a, b) not in have]
    assert not missing, missing
    kinds = {op.name.split("(")[0] for op in all_ops() if op.family == "session"}
    assert kinds == {"session-begin", "session-next", "session-next_i16"}


def test_every_family_is_sandwiched_between_decodes():
    trip = {(s[0].name, s[1].name, s[2].name) for _, s in windows(3)}
    missing = []
    for ch in Q.CHS:
        k1 = f"decode-f32(tonal9/k1,{ch}ch)"
        afters = [f"decode-f32(tonal9/lib,{ch}ch)", f"decode_resident(tonal9,{ch}ch)", f"decode-f32(tonal9/k2,{ch}ch)"] if ch == 2 else \
            [f"decode_resident(tonal9,{ch}ch)"]
        for fam in Q.FAMILIES:
            cands = Q.by_family(ch, fam)
            xs = {op.name for op in cands}
            for after in afters:
                if not any((k1, x, after) in trip for x in xs):
                    missing.append((fam, ch, after))
            # the operation of X on tonal9b (and not on tonal9): by the clips an operation works on, not by its name
            on_b = {op.name for op in cands if "tonal9b" in op.clips and "tonal9" not in op.clips}
            if ch == 2:
                assert on_b or fam in ("switch", "refused"), f"{fam} has no operation on tonal9b"      # these two work on no clip
                for after in afters:
                    if on_b and not any((k1, x, after) in trip for x in on_b):
                        missing.append((fam, "on tonal9b", after))
            for hook in (f"hook-compact_store({ch}ch)", f"hook-compact_batch({ch}ch)"):
                for after in afters:
                    if (k1, hook, after) not in trip:
                        missing.append((hook, after))
    assert not missing, missing


def test_the_plan_cache_patterns_exist():
    for ch in Q.CHS:
        A, B, big = f"decode-f32(tonal9/lib,{ch}ch)", f"decode-f32(tonal9b/lib,{ch}ch)", f"decode-f32(tonal130/lib,{ch}ch)"
        rng, im = f"decode_range-f32(tonal9,1..8,{ch}ch)", f"imdct_device+overlap_add(tonal9,1..9,{ch}ch)"
        im0 = f"imdct_device+overlap_add(tonal9,0..8,{ch}ch)"
        want = [[A, A], [A, B, A], [A, rng, A], [A, im, A], [A, im0, A], [A, "switch-imdct=5", A, "switch-imdct=0", A], [A, "switch-imdct=1", A, "switch-imdct=0", A],
                [A, big, A]]
        for pat in want:
            assert any([op.name for op in s] == pat for _, s in windows(len(pat))), pat
        # ... and the same launch count at another row_begin directly behind it, with no whole decode in between
        assert any([op.name for op in s] == [im, im0] for _, s in windows(2))


def test_every_family_interrupts_a_session():
    quad = {tuple(op.name for op in s) for _, s in windows(4)}
    begin = "session-begin(long1001,1ch)"
    closing = {"decode", "decode_dev", "decode_batch", "roundtrip", "roundtrip_batch", "compact_decode", "crops", "store_encode", "store_draw",
               "stream_encode", "stream_decode"}
    for fam in Q.FAMILIES:
        hits = [q for q in quad if q[0] == begin and q[1] == "session-next" and q[3] == "session-next" and Q.ops(1)[q[2]].family == fam]
        assert hits, fam
        for q in hits:
            res = Q.model_run([Q.ops(1)[n] for n in q])
            assert res[1][0] == 0 and res[1][2] == 0           # the first chunk, and it is not the last
            if fam in closing:
                assert res[3][0] == EINVAL, q
            elif fam in ("encode", "encode_batch", "encode_dev", "switch") + Q.MOVERS:
                assert res[3][0] == 0 and res[3][3][1] == "window", q        # the session survives: exactly the oracle's chunk
    for x in ("hook-compact_store(1ch)", "hook-compact_batch(1ch)", "switch-stream=1"):      # they leave the session open
        q = (begin, "session-next", x, "session-next")
        assert q in quad, x
        res = Q.model_run([Q.ops(1)[n] for n in q])
        assert res[3][0] == 0 and res[3][3][1] == "window"
    assert (begin, "session-next", "switch-stream=1", "session-next", "switch-stream=0", "session-next") in {tuple(op.name for op in s) for _, s in windows(6)}
    assert any(q[:3] == (begin, "session-next", "session-next_i16") for q in quad)
    res = Q.model_run([Q.ops(1)[n] for n in (begin, "session-next", "session-next_i16", "session-next")])
    assert res[2][0] == EINVAL and res[3][0] == 0             # formats do not mix, and the refusal costs the session nothing


def stepped(seq):
    """(operation, its modelled result, its lane before, its lane after) along a sequence on a fresh context."""
    st, out = Q.State(), []
    for op in seq:
        lanes = (st.enc if op.lane[0] == "enc" else st.dec) if op.lane else None
        before = dict(lanes[op.lane[1]]) if lanes is not None and op.lane[1] in lanes else None
        res = tuple(op.step(st, None))
        out.append((op, res, before, dict(lanes[op.lane[1]]) if lanes is not None else None))
    return out


def frames_behind(kind, ln):
    import stream_encode_cases as SE
    if ln is None:
        return 0
    if kind == "dec":
        return ln["at"]
    return Q.FRAMES[ln["name"]] if ln["finished"] else SE.frames_done(ln["at"])


def test_every_family_interrupts_a_lane():
    """"push, X, push" on an encoder lane and on a decoder lane, for every family X: the first push leaves the lane in
    mid-clip (samples held back, or a carry), X is no operation of that lane, and the model predicts for the second push
    bytes of the oracle - frames completed from what the lane held, no "stale" symbol."""
    seen = set()
    for name, seq in Q.sequences():
        run = stepped(seq)
        for (a, ra, _, mid), (x, _, _, _), (b, rb, before, after) in zip(run, run[1:], run[2:]):
            if a is not b or a.lane is None or x.lane == a.lane or not Q.is_mid_clip(mid):
                continue
            kind = a.lane[0]
            assert before == mid, (name, a, x)                  # X has not touched the lane
            if frames_behind(kind, after) > frames_behind(kind, mid) and rb[0] == 0 and not any(Q.is_sym(v) and v[1] == "stale" for v in rb):
                seen.add((kind, x.family))
    missing = [(k, f) for k in ("enc", "dec") for f in Q.FAMILIES if (k, f) not in seen]
    assert not missing, missing
    hows = {(op.lane[0], op.lane[1][1]) for op in dict(Q.sequences())["lane-interrupts"] if op.lane}
    assert hows == {("enc", "host"), ("enc", "dev"), ("dec", "host"), ("dec", "dev")}


def test_the_chunk_and_push_plans_have_the_edges():
    """A chunk that completes no frame, one that ends exactly on a completion point, a finish; pushes of one and of two
    segments; host f32, device interleaved f32 and device planar S16 pushes; f32 and S16 outputs; every lane operation's
    whole plan runs in some sequence, the finish and the restart behind it included."""
    import ctx_sequence_lanes as LN
    import stream_encode_cases as SE
    plan = LN.enc_plan(Q.item(2, "tonal9").pc)
    offs = LN.offsets(plan)
    assert SE.frames_done(offs[1]) == 0 and offs[2] == 1536 and SE.frames_done(offs[2]) == 1 and SE.frames_done(offs[2] - 1) == 0
    assert sorted(len(p) for p in LN.dec_plan(9)) == [1, 1, 2]
    kinds = {op.name.split("(")[0] for op in all_ops() if op.lane}
    assert kinds >= {"stream_enc-host", "stream_enc-dev-il", "stream_enc-dev-s16", "stream_dec-host-f32", "stream_dec-host-i16", "stream_dec-dev-f32",
                     "stream_dec-dev-i16", "stream_dec-whole"}
    finished, restarted = set(), set()
    for name, seq in Q.sequences():
        for op, res, before, after in stepped(seq):
            if op.lane and after["finished"]:
                finished.add(op.name)
            if op.lane and before is not None and before["finished"] and before["name"] == after["name"]:
                restarted.add(op.name)
    lane_ops = {op.name for op in all_ops() if op.lane}
    assert finished == lane_ops, lane_ops - finished
    assert restarted >= {n for n in lane_ops if "lane0:tonal9," in n}


def test_small_large_small_for_every_family_with_a_large_operation():
    tri = [s for _, s in windows(3)]
    for ch in Q.CHS:
        for fam in Q.FAMILIES:
            if Q.by_family(ch, fam, size="large"):
                assert any(s[0] is s[2] and s[0].family == s[1].family == fam and s[0].size == "small" and s[1].size == "large" and s[0].ch == ch
                           for s in tri), (fam, ch)
    assert {f for f in Q.FAMILIES if Q.by_family(2, f, size="large")} >= {"encode", "encode_batch", "encode_dev", "decode", "decode_dev", "decode_batch",
                                                                        "roundtrip", "roundtrip_batch", "compact_decode", "crops", "store_encode",
                                                                        "store_draw", "store_compact", "store_join", "store_cut"}


def test_dirty_calls_directly_precede_clean_ones():
    seen = set()
    for name, seq in Q.sequences():
        res = Q.model_run(seq)
        for i in range(1, len(seq)):
            before, after = res[i - 1][-2], res[i][-2]         # the compact status record behind either call
            if not (Q.is_sym(before) and before[1] == "status" and Q.is_sym(after) and after[1] == "status"):
                continue
            if any(w[0] for w in before[2]) and not any(w[0] for w in after[2]) and seq[i - 1].family == seq[i].family:
                kind = seq[i].name.split("(")[0]
                seen.add(kind if seq[i].family == "hooks" else seq[i].family)
    assert seen >= {"compact_decode", "crops", "store_draw", "hook-rows_from_compact", "hook-rows_from_compact_window", "stream_decode"}, seen
    pairs = {(s[0].name.split(",")[0], s[1].name.split(",")[0]) for _, s in windows(2)}
    assert ("roundtrip-device(noise5", "roundtrip-device(tonal9") in pairs and ("roundtrip-host-f32(noise5", "roundtrip-host-f32(tonal9") in pairs
    assert ("roundtrip_batch-planar(2xnoise5..", "roundtrip_batch-planar(2xtonal9..") in pairs


def test_power_every_mutation_changes_a_modelled_result():
    base = {name: Q.model_run(seq) for name, seq in Q.sequences()}
    unnoticed = [m for m in Q.MUTATIONS if all(Q.model_run(seq, m) == base[name] for name, seq in Q.sequences())]
    assert not unnoticed, unnoticed
    assert len(Q.MUTATIONS) == 25
    new = {"stream_encode_keeps_resident", "stream_decode_keeps_resident", "store_compact_forgets", "store_join_forgets", "store_cut_forgets",
           "mover_clears_last_status", "stream_decode_leaves_last_status", "empty_push_keeps_last_status", "refused_push_moves_lane",
           "forgetting_call_resets_lanes"}
    assert new <= set(Q.MUTATIONS)


def test_the_growing_reserve_slip_is_unobservable():
    """See ctx_sequence_cases.EQUIVALENT_MUTATIONS: the reserve grows in the sequences (tonal130 behind the small clips),
    and keeping the plan across it changes no modelled result - the plan it would keep is never asked for again."""
    grew = False
    for name, seq in Q.sequences():
        st = Q.State()
        for op in seq:
            g0 = st.groups
            op.step(st, None)
            grew |= g0 != 0 and st.groups > g0
        assert Q.model_run(seq, "growing_reserve_keeps_plan") == Q.model_run(seq), name
    assert grew


def test_every_operation_runs_in_a_sequence():
    """No operation is defined that runs on fresh contexts only, and the calls that must leave a record alone run while
    there is one: the model's tail in front of them is no EINVAL."""
    used = {op.name for op in all_ops()}
    for ch in Q.CHS:
        unused = [n for n in Q.ops(ch) if n not in used]
        assert not unused, unused
    seen = set()
    for name, seq in Q.sequences():
        res = Q.model_run(seq)
        for i in range(1, len(seq)):
            rt, rtb, cd = (not (Q.is_sym(v) and v[1] == "einval") for v in res[i - 1][-4:-1])
            if rt and rtb and cd and (seq[i].family == "refused" or seq[i].name.startswith(("roundtrip-records", "hook-compact_"))):
                seen.add(seq[i].name.split("(")[0])
            if rt and rtb and cd and seq[i].family in Q.MOVERS:          # the three movers: the tail is unchanged behind them
                assert res[i][-4:] == res[i - 1][-4:], (name, seq[i])
                seen.add(seq[i].family)
    assert seen >= {f"refused-{f}" for f in Q.FAMILIES if f != "refused"} | {"roundtrip-records", "hook-compact_store", "hook-compact_batch"} | \
        set(Q.MOVERS), seen


def test_the_queued_runs_hold_the_newer_device_calls():
    """Runs of three or more device-only operations hold a device join, a device cut, an eviction and a device push of
    either kind; in one run a mover directly follows a store draw (the device has written rtb_tab), and in one a crops or
    batch call directly follows a mover (the uploaded image again)."""
    runs = [run for _, run in Q.queued_sequences()]
    assert all(len(r) >= 3 and all(op.device_only for op in r) for r in runs)

    def some(pred):
        return any(pred(r) for r in runs)
    for fam in ("store_join", "store_cut", "store_compact"):
        assert some(lambda r: any(op.family == fam for op in r)), fam
    assert some(lambda r: any("glc_stream_enc_push_device" in op.calls for op in r))
    assert some(lambda r: any("glc_stream_dec_push_device" in op.calls for op in r))
    assert some(lambda r: any(a.family == "store_draw" and b.family in Q.MOVERS for a, b in zip(r, r[1:])))
    assert some(lambda r: any(a.family in Q.MOVERS and b.family in ("crops", "roundtrip_batch") for a, b in zip(r, r[1:])))
    # ... and one run per channel count holds all of it together, with pushes that complete frames: the same encoder lane
    # operation at least three times, its decoder's likewise (the first chunk of a clip completes nothing)
    def whole(r, ch):
        names = [op.name for op in r]
        return (all(op.ch == ch for op in r) and {op.family for op in r} >= set(Q.MOVERS) | {"stream_encode", "stream_decode"} and
                any(a.family == "store_draw" and b.family in Q.MOVERS for a, b in zip(r, r[1:])) and
                any(a.family in Q.MOVERS and b.family in ("crops", "roundtrip_batch") for a, b in zip(r, r[1:])) and
                max(names.count(op.name) for op in r if "glc_stream_enc_push_device" in op.calls) >= 3 and
                max(names.count(op.name) for op in r if "glc_stream_dec_push_device" in op.calls) >= 3)
    for ch in Q.CHS:
        assert some(lambda r: whole(r, ch)), ch


def test_every_exported_entry_point_is_called_or_exempt():
    """Every function include/glc.h exports is called by an operation that runs in a sequence or is on the exempt list with
    its reason; a name either side does not know fails, so the next feature's entry points cannot stay outside."""
    import os
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    names = Q.exported(os.path.join(inc, "glc.h"))
    hooks = Q.exported(os.path.join(inc, "glc_debug.h"))
    assert len(names) > 100 and "glc_store_cut_device" in names and "glc_version" in names
    called = {c for op in all_ops() for c in op.calls}
    assert not called - names - hooks, sorted(called - names - hooks)
    assert not set(Q.EXEMPT) - names, sorted(set(Q.EXEMPT) - names)
    assert not set(Q.EXEMPT) & called, sorted(set(Q.EXEMPT) & called)
    assert all(len(r) > 10 for r in Q.EXEMPT.values())
    assert not names - called - set(Q.EXEMPT), sorted(names - called - set(Q.EXEMPT))
    assert all(op.calls for op in all_ops() if op.family != "refused")


def test_the_newer_expected_values_stay_in_the_budget():
    """Segment blobs, join and cut twins, evictions, lane spans: computed on first use, and all of them well under a minute
    on top of the pool's oracle work (which test_the_pool_is_what_its_names_say holds to its own budget)."""
    import ctx_sequence_lanes as LN
    for ch in Q.CHS:             # the pool's part: not counted here
        for n in ("tonal9", "tonal9b", "mixed13", "noise5", "one", "tonal130", "tonal9_i16"):
            Q.item(ch, n).blob_enc, Q.item(ch, n).dec
    LN._segs.clear()
    LN._stores.clear()
    LN.spent[0] = 0.0
    seen = set()
    for name, seq in Q.sequences():
        for op, res in zip(seq, Q.model_run(seq)):
            for v in res:
                if Q.is_sym(v) and v not in seen and v[1] in ("evict", "join", "nojoin", "cut", "nocut", "segs", "segstore", "span", "lanes_out"):
                    seen.add(v)
                    assert Q.materialise(v) is not None
    assert {v[1] for v in seen} >= {"evict", "join", "cut", "segs", "segstore", "span", "lanes_out"}
    assert LN.spent[0] < 45.0, LN.spent[0]


def test_the_suite_has_the_size_the_issue_asks_for():
    n_ops = sum(len(Q.ops(ch)) for ch in Q.CHS)
    n_steps = sum(len(s) for _, s in Q.sequences())
    assert n_ops >= 300 and 300 <= n_steps <= 2000 and len(Q.queued_sequences()) >= 10       # 1963 steps: the cap is the next hundred
    assert {op.family for op in all_ops()} == set(Q.FAMILIES)


# ------------------------------------------------------------------------------------------ GPU: the harness

class LazyStreams:
    def __init__(self, assets):
        self.a, self.c = assets, {}

    def __getitem__(self, key):
        if key not in self.c:
            ch, name, ident = key
            g = self.a.g
            if ident == "lib":           # the object glc_encode returned, on a context of the assets' own
                s = self.a.enc.encode(Q.item(ch, name).x, ch)
                assert s.to_bytes() == Q.item(ch, name).glc and s.stream_id >= 1 << 63
            else:
                parts = self[(ch, name, "lib")].parts()
                s = g.EncodedAudio.from_parts(parts, Q.K_ID(ch, ident[1] if isinstance(ident, tuple) else name))
            self.c[key] = s
        return self.c[key]


class Assets:
    """Device copies of the pool, shared by every context under test and made by none of them."""

    def __init__(self, g, torch):
        self.g, self.torch = g, torch
        self.enc = g.Encoder(Q.SR)
        self.streams = LazyStreams(self)
        self.c = {}
        self._side = None

    def _dev(self, key, make):
        if key not in self.c:
            t = self.torch.from_numpy(np.ascontiguousarray(make())).cuda()
            assert t.data_ptr() % 64 == 0
            self.c[key] = t
        return self.c[key]

    def raw(self, key, make):
        return self._dev(key, make)

    def x(self, ch, name):
        return self._dev(("x", ch, name), lambda: Q.item(ch, name).x)

    def ints(self, ch, name):
        return self._dev(("ints", ch, name), lambda: Q.item(ch, name).ints)

    def records(self, ch, name):
        return self._dev(("rec", ch, name), lambda: Q.item(ch, name).records)

    def coeffs(self, ch, name):
        return self._dev(("coef", ch, name), lambda: Q.item(ch, name).coeffs)

    def blob(self, ch, name):
        return self._dev(("blob", ch, name), lambda: Q.item(ch, name).blob)

    def store(self, ch):
        entries, lengths, nbytes = Q.host_store_tables(ch)

        def arena():
            img = np.zeros(nbytes, np.uint8)
            for e, n in zip(entries, Q.store_names(ch)):
                b = Q.item(ch, n).blob
                img[e[0]:e[0] + b.size] = b
            return img
        return (self._dev(("arena", ch), arena), self._dev(("entries", ch), lambda: np.array(entries, np.int64).reshape(-1, 4)),
                self._dev(("lengths", ch), lambda: np.array(lengths, np.int64)), max(lengths))

    def side_stream(self):
        if self._side is None:
            self._side = self.torch.cuda.Stream()
        return self._side


_assets = []


@pytest.fixture(scope="module")
def world():
    import torch
    g = Q.G()
    a = Assets(g, torch)
    _assets.append(a)
    yield g, torch, a
    a.streams.c.clear()
    a.c.clear()
    a.enc.close()


def tail(env, want_tail):
    """The three getters and the resident id.  A getter the model expects to refuse is asked with every clip count the
    pool uses: a stale record of any size would answer one of them."""
    g, L, h = env.g, env.g.lib, env.h
    _, w_rtb, w_cd, _ = want_tail
    info = g._lib.GlcRoundtripInfo()
    rc = L.glc_roundtrip_last_info(h, C.byref(info))
    rt = "EINVAL" if rc == EINVAL else (rc,) if rc else (info.n_frames, info.n_raw_frames, info.total_nnz, info.serialized_bytes)

    def ask(fn, struct, want, read):
        counts = Q.PROBE_COUNTS if want == "EINVAL" else (len(want),)
        for n in counts:
            arr = (struct * n)()
            rc = fn(h, arr, n)
            if rc == 0:
                return tuple(read(a) for a in arr)
            if rc != EINVAL:
                return (rc,)
        return "EINVAL"
    rtb = ask(L.glc_roundtrip_batch_last_info, g._lib.GlcRoundtripInfo, w_rtb, lambda i: (i.n_frames, i.n_raw_frames, i.total_nnz, i.serialized_bytes))
    cd = ask(L.glc_decode_compact_last_status, g._lib.GlcCompactStatus, w_cd, lambda s: (s.flags, s.n_bad_rows, s.first_bad_row))
    return rt, rtb, cd, int(L.glc_ctx_resident_stream(h))


def describe(got, want):
    if isinstance(got, bytes) and isinstance(want, bytes):
        if len(got) != len(want):
            return f"{len(got)} bytes, expected {len(want)}"
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        bad = np.flatnonzero(a != b)
        return f"{bad.size} of {a.size} bytes differ, first at byte {bad[0]}"
    return f"got {str(got)[:200]}, expected {str(want)[:200]}"


def compare(got, want_syms, assets, where):
    assert len(got) == len(want_syms), f"{where}: {len(got)} result elements, expected {len(want_syms)}"
    for k, (g_el, w) in enumerate(zip(got, want_syms)):
        if Q.is_sym(w) and w[1] == "window" and isinstance(g_el, np.ndarray):       # a chunk: the part the oracle knows
            off, known = Q.untrimmed_slice(Q.item(w[2], w[3]), w[4], w[5], w[6])
            g_el = g_el[off:off + known.size].tobytes()
        if Q.is_sym(w) and w[1] == "records" and isinstance(g_el, bytes) and len(g_el) == Q.item(w[2], w[3]).records.size:
            g_el = Q.records_specified(g_el, w[2], w[3])
        want = Q.materialise(w, assets)
        if isinstance(g_el, np.ndarray):
            g_el = g_el.tobytes()
        if isinstance(want, (list, tuple)) and isinstance(g_el, (list, tuple)):
            same = list(map(_plain, g_el)) == list(map(_plain, want))
        else:
            same = g_el == want
        assert same, f"{where}: element {k}: {describe(g_el, want)}"


def _plain(v):
    return [_plain(x) for x in v] if isinstance(v, (list, tuple)) else v


def where_of(seq_name, seq, i):
    return f"{seq_name}: operation {i} {seq[i].name} (after {[op.name for op in seq[max(0, i - 3):i]]})"


def run_sequence(g, torch, assets, seq_name, seq, contexts=None, deal=None, on_stream=None):
    """Every operation on its context, the host synchronising after each; every result and tail compared.
    deal(i) -> index of the context operation i goes to (each context has a model of its own)."""
    ctxs = contexts or [g.Decoder(2, Q.SR)]
    states = [Q.State() for _ in ctxs]
    envs = [Q.Env(g, torch, c, assets) for c in ctxs]
    for env, st in zip(envs, states):
        env.st = st
    try:
        for i, op in enumerate(seq):
            k = deal(i) if deal else 0
            if on_stream:
                on_stream(i, ctxs[k])
            want = tuple(op.step(states[k], None))
            want_tail = states[k].tail()
            fin = op.run(envs[k])
            assert g.lib.glc_ctx_synchronize(envs[k].h) == 0
            got = tuple(fin())
            t = tail(envs[k], tuple(Q.materialise(v, assets) for v in want_tail))
            compare(got + t, want + want_tail, assets, where_of(seq_name, seq, i))
            envs[k].keep.clear()
    finally:
        for env in envs:
            env.close()
        if not contexts:
            for c in ctxs:
                c.close()


SEQ_NAMES = [n for n, _ in Q.sequences()]
QUEUED = Q.queued_sequences()


@gpu
@pytest.mark.parametrize("family", Q.FAMILIES)
def test_every_operation_alone(world, family):
    """Each operation on a context created for it: the harness, the expectations and the operations agree before anything
    is blamed on state."""
    g, torch, assets = world
    done = set()
    for ch in Q.CHS:
        for op in Q.ops(ch).values():
            if op.family == family and op.name not in done:
                done.add(op.name)
                run_sequence(g, torch, assets, "alone", [op])
    assert done


@gpu
@pytest.mark.parametrize("name", SEQ_NAMES)
def test_sequence_on_one_context(world, name):
    g, torch, assets = world
    run_sequence(g, torch, assets, name, dict(Q.sequences())[name])


@gpu
@pytest.mark.parametrize("name", [n for n, _ in QUEUED])
def test_sequence_queued_back_to_back(world, name):
    """Device entry points that do not synchronise, queued with nothing between them; every output, in a buffer of its
    own with the pattern around it, is compared after ONE glc_ctx_synchronize at the end."""
    g, torch, assets = world
    seq = dict(QUEUED)[name]
    ctx = g.Decoder(2, Q.SR)
    env = Q.Env(g, torch, ctx, assets)
    st = env.st = Q.State()
    try:
        pending = []
        for op in seq:
            want = tuple(op.step(st, None))
            pending.append((want, op.run(env)))
        assert g.lib.glc_ctx_synchronize(env.h) == 0
        for i, (want, fin) in enumerate(pending):
            compare(tuple(fin()), want, assets, where_of(name, seq, i))
        t = tail(env, tuple(Q.materialise(v, assets) for v in st.tail()))
        compare(t, st.tail(), assets, f"{name}: the getters behind the last operation")
    finally:
        env.close()
        ctx.close()


@gpu
def test_sequence_on_a_callers_stream(world):
    """One mixed sequence with the context on a torch side stream, and back on its own stream half way through."""
    g, torch, assets = world
    seq = [op for op in dict(Q.sequences())["walk-2ch"] if not op.name.startswith("switch-stream")]
    side = torch.cuda.Stream()
    half = len(seq) // 2

    def on_stream(i, ctx):
        if i == 0:
            ctx.set_stream(side.cuda_stream)
        elif i == half:
            ctx.set_stream(0)
    run_sequence(g, torch, assets, "walk-2ch on a caller's stream", seq, on_stream=on_stream)


@gpu
def test_two_contexts_interleaved(world):
    """The same sequence dealt alternately to two contexts of the same rate: each gives what its own model says - nothing
    process-wide (pinned images, the id counter) leaks from one to the other.  Both contexts hold an open stream encoder
    and an open stream decoder in mid-clip, host and device lanes, while the other runs its operations: every lane
    operation comes in pairs, one for each context, in front of the walk, between its two parts and behind it."""
    g, torch, assets = world
    o = Q.ops(3)
    lanes = [o["stream_enc-dev-il(lane0:tonal9,3ch)"], o["stream_dec-dev-f32(lane0:tonal9,3ch)"], o["stream_enc-host(lane1:tonal9b,3ch)"],
             o["stream_dec-host-i16(lane1:tonal9b,3ch)"]]
    pairs = [op for op in lanes for _ in range(2)]
    open_lanes = pairs + [op for op in lanes[:2] for _ in range(2)]          # two pushes on the device lanes: samples held back, a carry
    seq = open_lanes + dict(Q.sequences())["walk-3ch"] + pairs + dict(Q.sequences())["plan-cache-3ch"] + pairs
    st = [Q.State(), Q.State()]
    for i, op in enumerate(open_lanes):
        op.step(st[i % 2], None)
    assert all(Q.is_mid_clip(s.enc[k]) for s in st for k in s.enc) and all(Q.is_mid_clip(s.dec[k]) for s in st for k in s.dec)
    assert all(len(s.enc) == 2 and len(s.dec) == 2 for s in st) and len(open_lanes) % 2 == 0
    ctxs = [g.Decoder(3, Q.SR), g.Decoder(3, Q.SR)]
    try:
        run_sequence(g, torch, assets, "walk-3ch + plan-cache-3ch on two contexts", seq, contexts=ctxs, deal=lambda i: i % 2)
    finally:
        for c in ctxs:
            c.close()
