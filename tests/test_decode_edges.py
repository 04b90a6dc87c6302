"""The decode kernels at their structural edges (tests/decode_edges.py builds the streams).

CPU: the generator is deterministic, the C oracle and the numpy oracle agree on every block and on the decoded
PCM, the families reach the edges they claim (computed from the streams, so that an edit of the generator
cannot silently drop one), the expected outputs hold the answers that can be stated without an oracle, and a
numpy model of the shipped algorithm equals the oracles on every run while each of its single-edit mutations
(the kind of edit a kernel change could make) changes at least one expected output - so the GPU tests below
would notice them.  GPU: every run of every case through the shipped path into sentinel-filled buffers, every
float compared bit for bit (NaNs included: the MI355X gives the oracle's NaN bits, see
test_gpu_parity.py::test_infinite_scale_with_stored_zero) and the floats around each destination untouched;
the cross-check variants against the same bits; the reuse sequence; argument checks at their bounds; and the
overlap-add alone, through glc_debug_overlap_add_device (include/glc_debug.h), on blocks no decode can produce."""
import ctypes as C

import numpy as np
import pytest

import decode_edges as D
from decode_edges import FRAME, G, HOP, Run, bits
from oracle import glc_oracle_np as N
from oracle import oracle as O

F32 = np.float32
WHOLE_DECODE_ROWS = 300   # both oracles decode the whole stream for cases of at most this many rows


@pytest.fixture(scope="module")
def cases():
    return D.cases()


def _by_name(cs):
    return {c.name: c for c in cs}


def _family(cs, fam):
    return [c for c in cs if c.family == fam]


def _streams(c):
    return [c.stream] + ([c.info["other"]] if "other" in c.info else [])


def _steps(c):
    """(stream, run) of every run of a case."""
    if "steps" in c.info:
        return [(c.stream if s == "a" else c.info["other"], r) for s, r in c.info["steps"]]
    return [(c.stream, r) for r in c.runs]


# ----------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------

def test_generator_is_deterministic(cases):
    assert D.digest(D.build_cases()) == D.digest(cases)
    assert len({c.name for c in cases}) == len(cases)


def test_c_oracle_and_numpy_oracle_agree_on_every_case(cases):
    """Blocks: imdct_block (C) against imdct_rows (numpy) on every distinct row of every stream.  PCM: the
    overlap-add of the expected blocks against BOTH oracles' decode of the whole stream, un-trimmed (every hop
    range is a slice of it) and, for four families, trimmed; streams of more than WHOLE_DECODE_ROWS rows (placement, the long
    overlap stream) are made of the same few hundred distinct rows and are covered by the block comparison."""
    rows = {}
    for c in cases:
        for st in _streams(c):
            for f in range(st.nf):
                if st.raw[f] is None:
                    for r in st.rows[f * st.ch:(f + 1) * st.ch]:
                        rows.setdefault(r.key, r)
    D.row_blocks(rows.values())
    T, w, norm = N.tables_cached()
    keys = list(rows)
    with np.errstate(all="ignore"):
        co = np.stack([rows[k].coefficients() for k in keys])
        got = N.imdct_rows(co, T, norm) * w[None, :]
    for k, b in zip(keys, got):
        assert np.array_equal(bits(b), bits(D._block_cache[k])), f"row of {len(rows[k])} pairs, scale {rows[k].scale!r}"
    n_whole = 0
    for c in cases:
        for st in _streams(c):
            if st.nf * st.ch > WHOLE_DECODE_ROWS:
                continue
            n_whole += 1
            want_all = D.expected_hops(st, 0, st.nf + 1)
            full = D.Stream(st.sr, st.ch, st.rows, st.raw, delay=0, lose=0)
            assert full.orig == want_all.size
            with np.errstate(all="ignore"):
                for name, dec in (("C", O.decode(full.to_glc())[0]), ("numpy", N.decode(full.to_glc()))):
                    assert np.array_equal(bits(dec), bits(want_all)), f"{c.name}: {name} oracle, un-trimmed"
                if c.family in ("raw", "values", "reuse", "overlap"):   # the gapless window is the same rule everywhere
                    for name, dec in (("C", O.decode(st.to_glc())[0]), ("numpy", N.decode(st.to_glc()))):
                        assert np.array_equal(bits(dec), bits(D.trim(st, want_all))), f"{c.name}: {name} oracle, trimmed"
            for s_, r in _steps(c):
                if r.kind == "range" and s_ is st:
                    lo, hi = r.a * HOP * st.ch, r.b * HOP * st.ch
                    assert np.array_equal(bits(D.expected_run(st, r)), bits(want_all[lo:hi])), (c.name, r)
    assert n_whole >= 30
    # the known disagreement this module's values family exists for: a NaN scale is clamped like any other
    assert np.isfinite(D._block_cache[_by_name(cases)["values"].stream.rows[len(D.SCALES) - 1].key]).all()


def _launch_units(st, run):
    """(launch frames, batch index, [plan of each unit]) of every plan batch a run launches."""
    for a, b in D.launches_of(st, run):
        for i, (g0, n_fg) in enumerate(D.launch_batches(b - a, st.ch, D.plan_groups_of(st))):
            yield (a, b), i, [D.unit_plan(D.unit_rows(st, a, b, g0 + u // st.ch, u % st.ch)) for u in range(n_fg * st.ch)]


def test_families_cover_what_they_claim(cases):
    by = _by_name(cases)
    assert {c.family for c in cases} == {"union", "lists", "groups", "raw", "values", "placement", "reuse", "overlap"}

    # union: every n_u as a dense and as a split unit, the scan's boundaries, every skip state of every row pair
    for shape, dense in (("dense", True), ("split", False)):
        c = by[f"union-{shape}"]
        (_, _, plans), = list(_launch_units(c.stream, c.runs[0]))
        assert [p["n_u"] for p in plans[:len(D.UNION_SIZES)]] == list(D.UNION_SIZES)
        assert all(p["dense"] == (dense or p["n_u"] == 0) for p in plans[:len(D.UNION_SIZES)])
        seen = set(np.concatenate([p["union"] for p in plans]).tolist())
        assert set(D.SCAN_EDGES) <= seen
        for p in plans[:len(D.UNION_SIZES)]:
            if p["n_u"] >= 12:
                assert set(D.SCAN_EDGES) <= set(p["union"].tolist())
            if shape == "split":
                assert (p["owners"] == 1).all()             # every entry present in exactly one row
                if p["n_u"] >= G:
                    assert all(s == {(0, 0), (1, 0), (0, 1)} for s in p["states"]), p["n_u"]
            else:
                assert (p["owners"] == G).all()
        states = [set().union(*[p["states"][k] for p in plans]) for k in range(G // 2)]
        assert all(s >= ({(1, 1)} if dense else {(0, 0), (1, 0), (0, 1)}) for s in states)
        z = plans[c.info["zero_group"]]                      # stored zeros only: a union with nothing to apply
        assert z["n_u"] > 0 and (z["owners"] == 0).all()
        assert {r.kind for r in c.runs} == {"imdct", "decode"}

    # lists: every length beside empty and beside full rows, the long row at every position
    c = by["lists"]
    (_, _, plans), = list(_launch_units(c.stream, c.runs[0]))
    marks = c.info["marks"]
    for g, pos, L, nb in marks:
        lens = plans[g]["lens"]
        assert lens[pos] == L and all(x == (1024 if nb == "full" else 0) for i, x in enumerate(lens) if i != pos)
    assert {(L, nb) for _, _, L, nb in marks} >= {(L, nb) for L in D.LIST_LENGTHS for nb in ("empty", "full")}
    assert {pos for _, pos, L, nb in marks if (L, nb) == (257, "full")} == set(range(G))
    assert {pos for _, pos, L, nb in marks if (L, nb) == (513, "empty")} == set(range(G))

    # groups: frame counts, range starts, one-frame ranges, raw masks, channel counts
    fam = _family(cases, "groups")
    assert {c.stream.nf for c in fam} >= set(D.GROUP_FRAMES)
    assert {c.stream.ch for c in fam} == set(D.GROUP_CHANNELS)
    starts, ones, rem, masks, last_only = set(), set(), set(), {}, set()
    for c in fam:
        st = c.stream
        for r in c.runs:
            if r.kind != "imdct":
                continue
            starts.add(r.a)
            rem.add((r.b - r.a) % G)
            if r.b - r.a == 1:
                ones.add(r.a)
            for (a, b), _, plans in _launch_units(st, r):
                for u, p in enumerate(plans):
                    masks.setdefault(st.ch, set()).add((p["rawm"], p["live"]))
                raw_groups = {(f - a) // G for f in range(a, b) if st.raw[f] is not None}
                if raw_groups == {(b - a - 1) // G} and (b - a) % G:
                    last_only.add(st.ch)
    assert starts >= {0, *D.RANGE_STARTS} and ones >= set(D.RANGE_STARTS) and rem == set(range(G))
    for ch in (1, 3, 8):
        m = {rawm for rawm, _ in masks[ch]}
        assert m >= {1 << g for g in range(G)} | {0, 0xFF}, f"{ch} channels: raw masks {sorted(m)}"
        assert any(bin(x).count("1") == G - 1 for x in m)
        assert all(rawm & live == 0 for rawm, live in masks[ch])
    assert last_only >= {2, 5}

    # raw: vector lengths, values, channel counts
    fam = _family(cases, "raw")
    assert [c.stream.ch for c in fam] == list(D.RAW_CHANNELS)
    for c in fam:
        ch, st = c.stream.ch, c.stream
        sizes = [r.size for r in st.raw if r is not None]
        assert sizes[:6] == [0, 1, ch, FRAME * ch - 1, FRAME * ch, FRAME * ch + 1] == c.info["lengths"]
        vals = set(np.concatenate([r for r in st.raw if r is not None]).tolist())
        assert vals >= set(D.RAW_VALUES)
        if ch == 7:
            assert vals == set(range(-32768, 32768))
        assert {r.kind for r in c.runs} == {"imdct", "decode", "range"}

    # values: q at the ends of int16 under every scale, stored zeros
    c = by["values"]
    rows = c.stream.rows
    got_scales = [r.scale for r in rows[:len(D.SCALES)]]
    assert np.array_equal(bits(got_scales), bits(D.SCALES)) and len(D.SCALES) == 9
    assert np.isnan(D.SCALES[8]) and np.isinf(D.SCALES[7]) and 0 < D.SCALES[2] < np.finfo(np.float32).tiny
    assert D.SCALES[3] < D.TINY == D.SCALES[4] < D.SCALES[5] and bits(D.SCALES[5]) - bits(D.SCALES[3]) == 2
    assert all(set(r.q.tolist()) == set(D.Q_VALUES) for r in rows[:len(D.SCALES)])
    assert {(int(r.q[0]), bool(np.isinf(r.scale))) for r in rows if len(r) and r.q[0] == 0} == {(0, False), (0, True)}
    assert D.smallest_product() > 1e-21 > float(np.finfo(np.float32).tiny)   # no product can be subnormal

    # placement: units per plan batch, all ties / no ties, the second batch, variants 5 and 6
    seen = {}
    for c in _family(cases, "placement"):
        st = c.stream
        batches = [plans for _, _, plans in _launch_units(st, c.runs[0])]
        work = [[p["work"] for p in plans] for plans in batches]
        kinds = {"ties" if len(set(w)) == 1 else "alldiff" if len(set(w)) == len(w) else "mixed" for w in work}
        assert kinds == {c.info["kind"]}, (c.name, kinds)
        seen.setdefault(c.info["kind"], []).append([len(w) for w in work])
        for plans in batches:       # neighbouring units hold different rows: a misplaced unit shows
            keys = [tuple(p["lens"]) + tuple(p["union"].tolist()) for p in plans]
            assert all(a != b for a, b in zip(keys, keys[1:]))
    for kind in ("ties", "alldiff"):
        assert seen[kind] == [[u] for u in D.PLACEMENT_UNITS] + [[292 * 7, 7]], seen[kind]
    assert D.PLAN_GROUPS // D.TWO_BATCH[0] == 292 and D.PLAN_GROUPS % D.TWO_BATCH[0] != 0 and D.TWO_BATCH[1] % G != 0
    v = {(r.variant, c.info["units"], c.stream.ch) for c in _family(cases, "placement") for r in c.runs if r.variant}
    assert v == {(6, 1023, 3), (6, 1025, 5), (5, 1024, 4), (5, 2048, 8)}
    assert all(256 % ch for var, _, ch in v if var == 6) and all(u % 256 == 0 and u % ch == 0 for var, u, ch in v if var == 5)

    # reuse: the same launch twice, another range, back, another variant, back, another stream of the same shape, halo + one frame
    c = by["reuse"]
    steps, a, b = c.info["steps"], c.stream, c.info["other"]
    key = [(s, r.kind, r.a, r.b, r.variant) for s, r in steps]
    assert key[0] == key[1] and key[2][2:4] != key[0][2:4] and key[3] == key[0] and key[4][4] == 2 and key[5] == key[0]
    assert key[6][0] == "b" and key[6][1:] == key[0][1:] and key[8] == key[0]
    assert key[9][1:4] == ("range", 5, 6) and key[10][1:4] == ("imdct", 4, 5)
    pa, pb = [len(r) for r in a.rows], [len(r) for r in b.rows]
    assert pa == pb and [None if r is None else r.size for r in a.raw] == [None if r is None else r.size for r in b.raw]
    assert a.to_glc() != b.to_glc() and len(a.to_glc()) == len(b.to_glc())

    # overlap: hop ranges at both ends, pointer offsets for every channel count, the decode round's boundary
    fam = _family(cases, "overlap")
    assert [c.stream.ch for c in fam[:-1]] == list(D.OVERLAP_CHANNELS)
    for c in fam[:-1]:
        nf = c.stream.nf
        rr = {(r.a, r.b) for r in c.runs if r.kind == "range"}
        assert rr >= {(0, 1), (0, nf + 1), (nf, nf + 1), (nf - 1, nf + 1)} and any(a == b for a, b in rr)
        assert {r.offset for r in c.runs if (r.a, r.b) == (0, nf + 1)} == set(D.OFFSETS)
    assert {r.offset for c in fam[:-1] for r in c.runs if r.kind == "range" and r.b - r.a == 1} == set(D.OFFSETS)
    c = fam[-1]
    R = D.ROUND_FRAMES
    assert c.stream.nf > R + 1 and {r.b for r in c.runs if r.kind == "range"} >= {R - 1, R, R + 1, R + 2, c.stream.nf + 1}
    assert any(len(D.launches_of(c.stream, r)) >= 2 and r.a == 0 for r in c.runs)       # a second round
    assert any(len(D.launches_of(c.stream, r)) >= 3 and r.a > 0 for r in c.runs)        # halo + two rounds


def test_expected_outputs_hold_the_known_answers(cases):
    by = _by_name(cases)
    zero = np.zeros(FRAME, np.uint32)
    for shape in ("dense", "split"):
        c = by[f"union-{shape}"]
        blk = D.expected_blocks(c.stream, 0, c.stream.nf)
        assert all(np.array_equal(bits(b), zero) for b in blk[:G])                    # empty union: +0.0 everywhere
        z = c.info["zero_group"] * G
        assert all(np.array_equal(bits(b), zero) for b in blk[z:z + G])               # only stored zeros, finite scale
        assert all(bits(b).any() for b in blk[G:2 * G] if shape == "dense")
    for c in _family(cases, "raw"):
        st = c.stream
        blk = D.expected_blocks(st, 0, st.nf).reshape(st.nf, st.ch, FRAME)
        assert not bits(blk[1]).any()                                                 # raw_len = 0: +0.0
        assert blk[2, 0, 0] == F32(st.raw[2][0]) / F32(32767.0) and not bits(blk[2]).reshape(-1)[1:].any()
        f = 8                                                                         # the int16 extremes, interleaved
        v = st.raw[f].reshape(FRAME, st.ch)
        assert np.array_equal(blk[f], (v.T.astype(np.float64) / 32767.0).astype(F32))
        assert F32(-32768.0) / F32(32767.0) in blk[f] and F32(1.0) in blk[f] and blk[f].min() < -1.0
        assert not bits(blk[4, st.ch - 1, FRAME - 1]).any()   # one sample short
        for f in (5, 6):                                                              # exact length; one sample too many
            v = st.raw[f][:FRAME * st.ch].reshape(FRAME, st.ch)
            assert np.array_equal(blk[f], (v.T.astype(np.float64) / 32767.0).astype(F32))
    c = by["values"]
    blk = D.expected_blocks(c.stream, 0, c.stream.nf)
    for i in (0, 1, 2, 3, 8):                    # 0, -1, subnormal, just under 1e-12 and NaN all clamp to 1e-12
        assert np.array_equal(bits(blk[i]), bits(blk[4])), repr(D.SCALES[i])
    assert not np.array_equal(bits(blk[5]), bits(blk[4])) and np.isfinite(blk[:6]).all() and np.abs(blk[4]).max() < 1e-12
    names = c.info["names"]
    assert np.isfinite(blk[names.index("stored zero, finite scale")]).all()
    assert np.isnan(blk[names.index("stored zero, infinite scale")]).all()
    assert np.isnan(blk[names.index("only a stored zero, infinite scale")]).all()
    for c in _family(cases, "overlap")[:-1]:
        st, nf = c.stream, c.stream.nf
        blk = D.expected_blocks(st, 0, nf).reshape(nf, st.ch, FRAME)
        tail = D.expected_run(st, Run("range", nf, nf + 1))
        assert np.array_equal(bits(tail), bits(blk[nf - 1, :, HOP:].T.reshape(-1)))   # the bare tail: a copy
        hop0 = D.expected_run(st, Run("range", 0, 1))
        assert np.array_equal(bits(hop0), bits((F32(0.0) + blk[0, :, :HOP]).T.reshape(-1)))
        assert D.expected_run(st, Run("range", 2, 2)).size == 0


_HINT = {"drop_tail": "union", "first_256_pairs": "lists", "union_7_rows": "union", "pair_skip_either": "union",
         "no_clamp": "values", "nan_through_clamp": "values", "past_end_live": "groups", "raw_le": "raw",
         "raw_planar": "raw", "raw_mul_recip": "raw", "norm_times_window": "union", "rank_tie_le": "placement",
         "tail_added": "overlap", "hop0_reads_prev": "overlap"}


def _differs(st, run, mut):
    with np.errstate(all="ignore"):
        return not np.array_equal(bits(D.model_run(st, run, mut)), bits(D.expected_model_run(st, run)))


def test_power_the_model_equals_the_oracle_and_every_mutation_shows(cases):
    """The numpy model of the shipped algorithm gives the expected bits on every run of every case (spare frames
    behind an imdct range untouched), and every mutated copy of it changes the expected output of some run -
    which is what makes the GPU tests below able to catch such an edit of a kernel or of the launch code."""
    for c in cases:
        for st, run in _steps(c):
            assert not _differs(st, run, None), (c.name, run)
    assert len(D.MUTATIONS) >= 10 and set(_HINT) == set(D.MUTATIONS)
    caught = {}
    for mut in D.MUTATIONS:
        for c in _family(cases, _HINT[mut]):
            hit = [run for st, run in _steps(c) if _differs(st, run, mut)]
            if hit:
                caught.setdefault(mut, []).append((c.name, len(hit)))
    missed = [m for m in D.MUTATIONS if m not in caught]
    assert not missed, f"mutations no expected output notices: {missed}"
    names = {m: {n for n, _ in v} for m, v in caught.items()}
    # a wrong tie-break shows wherever the units are ranked (more than 256) and tied, below and above rank 1024
    assert names["rank_tie_le"] >= {f"placement-ties-{u}" for u in (257, 1023, 1024, 1025, 2047, 2048, 2051)}
    assert names["drop_tail"] == {"union-dense", "union-split"} and names["first_256_pairs"] == {"lists"}
    assert names["raw_le"] == {f"raw-ch{ch}" for ch in D.RAW_CHANNELS}
    assert names["raw_planar"] == {f"raw-ch{ch}" for ch in D.RAW_CHANNELS if ch > 1}   # one channel: planar is interleaved


# ----------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------

PAD = 4096   # sentinel floats in front of every destination (a multiple of 4: the pad keeps the 16-byte phase)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    import glc_amd
    f = glc_amd.lib.glc_debug_set_imdct_variant
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int]
    f = glc_amd.lib.glc_debug_overlap_add_device
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_uint16, C.c_uint64, C.c_uint64,
                  C.c_void_p, C.c_uint64]
    return torch, glc_amd


def _sentinel_tensor(torch, n):
    t = torch.full((n,), D.SENTINEL_BITS, dtype=torch.int32, device="cuda")
    assert t.data_ptr() % 16 == 0
    return t


def _explain(got, exp, per_row):
    bad = np.flatnonzero(got != exp)
    unwritten = int((got[bad] == D.SENTINEL_BITS).sum())
    rows = np.unique(bad // per_row)
    return (f"{bad.size} of {exp.size} floats differ ({unwritten} never written) in {rows.size} rows of {per_row}; "
            f"first: row {bad[0] // per_row} column {bad[0] % per_row}, got {got[bad[0]]:#010x} want {exp[bad[0]]:#010x}; "
            f"rows {rows[:12].tolist()}")


def _check_buffer(buf, at, exp, per_row, what):
    """buf (uint32, from the device): `exp` at [at, at + exp.size), the sentinel everywhere else."""
    e = bits(exp)
    assert (buf[:at] == D.SENTINEL_BITS).all(), f"{what}: floats in front of the destination were written"
    rest = buf[at + e.size:]
    assert (rest == D.SENTINEL_BITS).all(), \
        f"{what}: {int((rest != D.SENTINEL_BITS).sum())} floats behind the destination were written, first at +{int(np.flatnonzero(rest != D.SENTINEL_BITS)[0])}"
    got = buf[at:at + e.size]
    assert np.array_equal(got, e), f"{what}: {_explain(got, e, per_row)}"


def _set_variant(gpu, dec, v):
    assert gpu[1].lib.glc_debug_set_imdct_variant(dec._h, v) == 0


def _run(gpu, dec, ea, st, run, what, variant=None):
    """One run on the device into a sentinel-filled buffer; every float compared."""
    torch, glc_amd = gpu
    v = run.variant if variant is None else variant
    _set_variant(gpu, dec, v)
    exp = D.expected_run(st, run)
    what = f"{what} {run.kind}[{run.a}, {run.b}) offset {run.offset} variant {v}"
    try:
        if run.kind == "decode":
            out = D.sentinel(exp.size + 64).copy()
            got = dec.decode(ea, out=out)
            assert got.size == exp.size, what
            _check_buffer(out.view(np.uint32), 0, exp, HOP * st.ch, what)
            return
        spare = G * st.ch * FRAME if run.kind == "imdct" else PAD      # 8 frames: where a row past the range would land
        at = PAD + run.offset // 4
        d = _sentinel_tensor(torch, at + exp.size + spare)
        torch.cuda.synchronize()
        if run.kind == "imdct":
            dec.imdct_device(ea, run.a, run.b, d.data_ptr() + 4 * at)
        else:
            dec.decode_range_device(ea, run.a, run.b, d.data_ptr() + 4 * at, exp.size)
        dec.synchronize()
        _check_buffer(d.cpu().numpy().view(np.uint32), at, exp, FRAME if run.kind == "imdct" else HOP * st.ch, what)
    finally:
        _set_variant(gpu, dec, 0)


def _case_ids(*families):
    return [c.name for c in D.cases() if c.family in families]


@pytest.mark.gpu
@pytest.mark.parametrize("name", _case_ids("union", "lists", "groups", "raw", "values", "placement", "overlap"))
def test_gpu_every_run_of_every_case(gpu, cases, name):
    c = _by_name(cases)[name]
    glc_amd = gpu[1]
    dec = glc_amd.Decoder(c.stream.ch, c.stream.sr)
    ea = c.stream.to_encoded(glc_amd, c.how)
    assert ea.info().n_frames == c.stream.nf
    for run in c.runs:
        _run(gpu, dec, ea, c.stream, run, name)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 2, 3, 4])
@pytest.mark.parametrize("name", _case_ids("union", "lists", "groups", "values"))
def test_gpu_cross_check_variants_give_the_expected_bits(gpu, cases, name, variant):
    c = _by_name(cases)[name]
    glc_amd = gpu[1]
    dec = glc_amd.Decoder(c.stream.ch, c.stream.sr)
    ea = c.stream.to_encoded(glc_amd, "bytes")
    for run in c.runs:
        _run(gpu, dec, ea, c.stream, run, name, variant)


@pytest.mark.gpu
def test_gpu_reuse_sequence(gpu, cases):
    """One Decoder through launches that repeat (the plan kernel is skipped), change range, variant and stream;
    every step against the oracle, not against the step before."""
    c = _by_name(cases)["reuse"]
    glc_amd = gpu[1]
    a, b = c.stream, c.info["other"]
    ea = {"a": a.to_encoded(glc_amd, "parts"), "b": b.to_encoded(glc_amd, "parts")}
    dec = glc_amd.Decoder(a.ch, a.sr)
    for i, (s, run) in enumerate(c.info["steps"]):
        _run(gpu, dec, ea[s], a if s == "a" else b, run, f"reuse step {i} stream {s}")
    # the same content under a caller-supplied identity: recognised as resident, decoded without a new plan
    e1, e2 = a.to_encoded(glc_amd, "nested", stream_id=77), a.to_encoded(glc_amd, "parts", stream_id=77)
    for i, e in enumerate((e1, e2, e1)):
        _run(gpu, dec, e, a, Run("imdct", 0, a.nf), f"reuse id step {i}")
        assert dec.resident_stream() == 77


@pytest.mark.gpu
def test_gpu_entry_points_check_their_bounds(gpu, cases):
    torch, glc_amd = gpu
    c = _by_name(cases)["groups-ch2-nf9"]
    st = c.stream
    nf, ch = st.nf, st.ch
    ea = st.to_encoded(glc_amd)
    dec = glc_amd.Decoder(ch, st.sr)
    d = _sentinel_tensor(torch, (nf + 2) * ch * FRAME)
    torch.cuda.synchronize()
    for f0, f1 in ((0, nf + 1), (nf, nf + 1), (3, 2), (nf + 1, nf + 1)):
        with pytest.raises(glc_amd.GlcError):
            dec.imdct_device(ea, f0, f1, d.data_ptr())
    for h0, h1, cap in ((0, nf + 2, 1 << 40), (nf + 1, nf + 2, 1 << 40), (3, 2, 1 << 40),
                        (0, nf + 1, (nf + 1) * HOP * ch - 1), (nf, nf + 1, HOP * ch - 1)):
        with pytest.raises(glc_amd.GlcError):
            dec.decode_range_device(ea, h0, h1, d.data_ptr(), cap)
    with pytest.raises(glc_amd.GlcError):
        dec.imdct_device(ea, 0, nf, 0)
    dec.synchronize()
    assert (d.cpu().numpy().view(np.uint32) == D.SENTINEL_BITS).all()   # a refused call writes nothing
    # and the bounds themselves are accepted
    _run(gpu, dec, ea, st, Run("imdct", nf, nf), "empty range at the end")
    _run(gpu, dec, ea, st, Run("imdct", nf - 1, nf), "last frame")
    _run(gpu, dec, ea, st, Run("range", nf + 1, nf + 1), "empty hop range at the end")
    _run(gpu, dec, ea, st, Run("range", 0, nf + 1), "all hops, cap exact")


# ---- D2 alone, on caller-supplied blocks --------------------------------------------------------------

_SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0xFFC00000, 0x00000001, 0x80000001, 0x007FFFFF,
                      0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32).view(F32)


def _special_blocks(rng, n_frames, ch):
    """Blocks of +-0.0, +-inf, NaN (one bit pattern: which of two different NaNs an add returns is not pinned by
    IEEE 754), subnormals, +-1, +-FLT_MAX and ordinary values, so that every pair of classes meets in some add."""
    b = rng.standard_normal((n_frames, ch, FRAME)).astype(F32)
    m = rng.random(b.shape) < 0.5
    b[m] = _SPECIALS[rng.integers(0, _SPECIALS.size, int(m.sum()))]
    return b


def _overlap_add_device(gpu, dec, blocks, blk_frame0, nf, ch, h0, h1, offset, what, expect_rc=0):
    torch, glc_amd = gpu
    d_blk = torch.from_numpy(blocks.reshape(-1).view(np.int32)).cuda()
    n = max(h1 - h0, 0) * HOP * ch
    at = PAD + offset // 4
    d = _sentinel_tensor(torch, at + n + PAD)
    torch.cuda.synchronize()
    rc = glc_amd.lib.glc_debug_overlap_add_device(dec._h, d_blk.data_ptr(), blk_frame0, blocks.shape[0], nf, ch, h0, h1,
                                                  d.data_ptr() + 4 * at, n)
    assert rc == expect_rc, (what, glc_amd.lib.glc_last_error(dec._h))
    dec.synchronize()
    return d.cpu().numpy().view(np.uint32), at


@pytest.mark.gpu
@pytest.mark.parametrize("blk_frame0", [-1, 0])
@pytest.mark.parametrize("ch", [1, 2, 3, 4, 8])
def test_gpu_overlap_add_on_supplied_blocks(gpu, ch, blk_frame0):
    """-0.0, inf, NaN and subnormal operands, the +0.0 + x of hop 0 on a -0.0 input, both store forms; blocks as
    the decode rounds hold them (slot 0 = the frame in front, blk_frame0 = -1) and from frame 0."""
    glc_amd = gpu[1]
    nf = 6
    rng = np.random.default_rng(900 + ch)
    frames = _special_blocks(rng, nf, ch)
    frames[0, :, :8] = F32(-0.0)                                   # hop 0: +0.0 + -0.0 = +0.0, not a copy
    blocks = frames if blk_frame0 == 0 else np.concatenate([D.sentinel((1, ch, FRAME)), frames])
    dec = glc_amd.Decoder(ch, 48000)
    want_all = D.overlap_add(frames.reshape(-1, FRAME), 0, nf, ch, 0, nf + 1)
    assert not bits(want_all[:8 * ch]).any() and np.isnan(want_all).any() and np.isinf(want_all).any()
    for h0, h1 in ((0, nf + 1), (1, nf + 1), (0, 1), (nf, nf + 1), (2, 5), (3, 3)):
        for offset in D.OFFSETS:
            what = f"{ch} channels, hops [{h0}, {h1}), offset {offset}, blk_frame0 {blk_frame0}"
            buf, at = _overlap_add_device(gpu, dec, blocks, blk_frame0, nf, ch, h0, h1, offset, what)
            _check_buffer(buf, at, want_all[h0 * HOP * ch:h1 * HOP * ch], HOP * ch, what)
    # arguments: hops past the tail, frames the blocks do not hold, a short destination, no channels
    E = -1  # GLC_EINVAL
    for args in ((0, nf + 2), (3, 2)):
        _overlap_add_device(gpu, dec, blocks, blk_frame0, nf, ch, *args, 0, "hop range", expect_rc=E)
    _overlap_add_device(gpu, dec, blocks[:-1], blk_frame0, nf, ch, 0, nf + 1, 0, "last frame not held", expect_rc=E)
    _overlap_add_device(gpu, dec, blocks, blk_frame0 + 2, nf, ch, 1, 3, 0, "first frame not held", expect_rc=E)
    _overlap_add_device(gpu, dec, blocks, -2, nf, ch, 0, 1, 0, "blk_frame0 < -1", expect_rc=E)
    torch = gpu[0]
    d = _sentinel_tensor(torch, 64)
    f = glc_amd.lib.glc_debug_overlap_add_device
    assert f(dec._h, d.data_ptr(), 0, nf, nf, ch, 0, 1, d.data_ptr(), HOP * ch - 1) == E
    assert f(dec._h, d.data_ptr(), 0, nf, nf, 0, 0, 1, d.data_ptr(), 1 << 30) == E
    assert f(dec._h, None, 0, nf, nf, ch, 0, 1, d.data_ptr(), 1 << 30) == E
    assert f(dec._h, d.data_ptr(), 0, nf, nf, ch, 0, 1, None, 1 << 30) == E


@pytest.fixture(scope="module")
def many_mono_blocks():
    rng = np.random.default_rng(990)
    small = _special_blocks(rng, 61, 1)
    return small[np.arange(32769) % 61] + np.arange(32769, dtype=F32)[:, None, None]     # every frame different


@pytest.mark.gpu
@pytest.mark.parametrize("hops", [32767, 32768, 32769])
def test_gpu_overlap_add_across_the_32768_hop_slab(gpu, many_mono_blocks, hops):
    """launch_overlap_add cuts a launch into slabs of 32768 hops (the grid's y extent is 16 bits); no decode entry
    point launches more than 4097.  Mono, `hops` hops of a stream of hops - 1 frames (the last hop is the bare
    tail); the largest case holds 0.27 GB of blocks and 0.13 GB of output on the device (about 0.4 GB)."""
    glc_amd = gpu[1]
    nf = hops - 1
    blocks = many_mono_blocks[:nf]
    dec = glc_amd.Decoder(1, 48000)
    b = blocks.reshape(nf, FRAME)
    want = np.empty((hops, HOP), F32)
    with np.errstate(all="ignore"):
        want[0] = F32(0.0) + b[0, :HOP]
        want[1:nf] = b[:-1, HOP:] + b[1:, :HOP]
        want[nf] = b[nf - 1, HOP:]
    for offset in (0, 4):
        what = f"{hops} hops, offset {offset}"
        buf, at = _overlap_add_device(gpu, dec, blocks, 0, nf, 1, 0, hops, offset, what)
        _check_buffer(buf, at, want.reshape(-1), HOP, what)
