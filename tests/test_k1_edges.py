"""The forward transform kernels at their value and layout edges (tests/k1_edges.py builds the cases).

CPU: the generator is deterministic; the C oracle and the numpy oracle agree bit for bit on a subset of rows of
every case that holds every station - except exactly the rows in which two different NaN patterns meet, which
the reference does not define; the families reach the row counts, tile positions and offsets they claim
(computed from the cases); the expected outputs hold the answers that need no oracle; a numpy model of the
transform equals the oracle, and each of its single-edit mutations - fused multiply-add, a second accumulator,
another order, flushed subnormals, a folded table, a wrong padding or channel rule - changes an expected word,
so the GPU tests below would notice such an edit of a kernel.

GPU: every case through every kernel it names (by row count, or pinned through glc_debug_set_mdct_variant), from a
shard with NaN on both sides into a sentinel-filled destination; ALL rows compared bit for bit with the oracle,
NaN bits included; the guards family again with 1 / 3 / 5 samples of extra halo; the far family also through
glc_encode_range_device, records byte for byte."""
import ctypes as C

import numpy as np
import pytest

import k1_edges as K
from k1_edges import FRAME, HOP, bits
from oracle import glc_oracle_np as N
from oracle import oracle as O

F32 = np.float32


@pytest.fixture(scope="module")
def cases():
    return K.cases()


@pytest.fixture(scope="module")
def subsets(cases):
    """name -> (rows, the C oracle's coefficients of those rows): at most 64 rows per case, computed once."""
    out = {}
    for c in cases:
        rows = K.subset_rows(c)
        assert 0 < rows.size <= 64
        out[c.name] = (rows, K.oracle_rows(c, rows))
    return out


def _by_name(cs):
    return {c.name: c for c in cs}


def _family(cs, fam):
    return [c for c in cs if c.family == fam]


def _differing_rows(a, b):
    return np.flatnonzero((bits(a) != bits(b)).any(axis=1))


# ----------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------

def test_generator_is_deterministic(cases):
    assert K.digest(K.build_cases()) == K.digest(cases)
    assert len({c.name for c in cases}) == len(cases)


def test_c_oracle_and_numpy_oracle_agree_except_where_two_nan_patterns_meet(cases, subsets):
    """mdct_block of the C oracle (through encode_range_records, its own loader) against mdct_rows of the numpy
    oracle on the windowed rows.  They must agree on every row but the unpinned stations' and DISAGREE on exactly
    those: both add a NaN product to a NaN sum there, and which payload comes out is the compiler's operand order."""
    T, w, norm = N.tables_cached()
    n_unpinned = 0
    for c in cases:
        rows, want = subsets[c.name]
        assert set(K.station_rows(c).values()) | set(K.unpinned_rows(c)) <= set(rows.tolist())
        with np.errstate(all="ignore"):
            got = N.mdct_rows(K.load_rows(c, rows) * w[None, :], T, norm)
        differ = rows[_differing_rows(got, want)].tolist()
        assert differ == K.unpinned_rows(c), f"{c.name}: the oracles differ in rows {differ}, unpinned are {K.unpinned_rows(c)}"
        un = np.isin(rows, K.unpinned_rows(c))
        assert np.array_equal(np.isnan(got[un]), np.isnan(want[un]))        # where the NaNs are is defined
        n_unpinned += int(un.sum())
    assert n_unpinned == 4 * len(_family(cases, "values"))


def test_families_reach_what_they_claim(cases):
    by = _by_name(cases)
    assert {c.family for c in cases} == {"values", "all_rows", "channels", "guards", "far"}
    for c in cases:      # every launch on the stated side of 640 / 1792 / 2048 / 3584 / 4096, by the dispatch's own rule
        seg = c.ch in K.SEG_CHANNELS
        for kernel, variant in c.targets:
            assert K.kernel_for(c.M, c.ch, variant) == kernel and variant == K.VARIANT.get(kernel, 0)
            lo, hi = {"small2": (1, 640), "sched": (1793, 2048), "small4": (641, 3583 if seg else 4095)}.get(
                kernel, (3584 if seg else 4096, 1 << 32))
            assert lo <= c.M <= hi, (c.name, kernel)
        cls = c.info["cls"]
        assert {k for k, _ in c.targets} == {"large": {"dma", "st8", "st16"}, "sched": {"sched", "small4"}}.get(cls, {cls})
        assert 0 <= c.f0 < c.f1 <= c.src.n_frames and c.M == (c.f1 - c.f0) * c.ch

    # all_rows: every row count of the table, both sides of every threshold, every loader shape of the large kernels
    fam = _family(cases, "all_rows")
    for cls, (seg, other) in K.TABLE.items():
        got_seg = sorted(c.M for c in fam if c.info["cls"] == cls and c.ch == 1)
        assert got_seg == sorted(seg), (cls, got_seg)
        got_other = sorted(c.M for c in fam if c.info["cls"] == cls and c.ch == 3)
        assert len(got_other) == len(other) and all(abs(a - b) < 3 for a, b in zip(got_other, sorted(other)))
    assert {c.ch for c in fam if c.info["cls"] == "large"} == {1, 2, 4, 8, 3}
    assert {c.M for c in fam if c.ch == 1} >= {640, 641, 1793, 2048, 3583, 3584} and {c.M for c in fam if c.ch == 3} >= {4095, 4098}
    assert all(c.f0 == 0 for c in fam) and any(c.f1 == c.src.n_frames and c.src.n_samples % c.ch for c in fam)

    # values: every kernel, both loaders of the large ones and 8 channels; stations where they should be
    fam = _family(cases, "values")
    reached = {(k, c.ch in K.SEG_CHANNELS) for c in fam for k, _ in c.targets}
    assert reached == {(k, s) for k in ("small2", "small4", "sched", "dma", "st8", "st16") for s in (True, False)}
    assert {c.ch for c in fam} == {2, 3, 8}
    for c in fam:
        st = K.station_rows(c)
        assert set(st) == set(K.STATIONS) and len(set(st.values())) == len(st) and max(st.values()) < K.STATION_LIMIT < c.M
        r = np.array(sorted(st.values()))
        assert {0, 31} <= set((r % 32).tolist()) and {0, 255} <= set((r % 256).tolist())   # first / last row of both tile heights
        assert 0 in r and {63, 127} & set((r % 128).tolist())
        where = sorted(divmod(x, c.ch)[::-1] for x in r)                 # (channel, frame)
        assert all(a[0] != b[0] or b[1] - a[1] >= 3 for a, b in zip(where, where[1:]))      # no row sees two stations
        u = bits(K.load_rows(c, r))
        names = [n for n, _ in sorted(st.items(), key=lambda kv: kv[1])]
        row = dict(zip(names, u))
        imp = {int(n[9:]): row[n] for n in names if n.startswith("impulse-i")}
        assert sorted(imp) == sorted(K.I_POS)
        for i, x in imp.items():
            assert np.flatnonzero(x).tolist() == [i]
        assert {int(x[i]) for i, x in imp.items()} == {K.word(1.0), K.word(-1.0)}
        tiny = np.finfo(F32).tiny
        assert (np.abs(row["subnormal-window"].view(F32)) < tiny).all() and row["subnormal-window"].all()
        mixed = np.abs(row["subnormal-mixed"].view(F32))
        assert (mixed[::2] < tiny).all() and (mixed[1::2] >= tiny).all()
        _, w, _ = O.tables()
        ends = row["tiny-at-ends"].view(F32) * w
        assert (np.abs(ends[:8]) < tiny).all() and ends[:8].all() and (np.abs(ends[-8:]) < tiny).all() and ends[-8:].all()
        assert (row["negative-zero"] == K.NEG_ZERO).all() and not row["zero"].any()
        assert set(np.unique(row["zero-signed-against-column-0"]).tolist()) == {0, K.NEG_ZERO}
        assert (np.abs(row["huge"].view(F32)) > 2.9e38).sum() >= 8
        for name, words in (("plus-inf", [K.PINF]), ("minus-inf", [K.NINF]), ("inf-minus-inf", [K.PINF, K.NINF]),
                            ("quiet-nan", [K.QNAN]), ("signalling-nan", [K.SNAN]), ("nan-then-inf-minus-inf", [K.QNAN, K.PINF, K.NINF]),
                            ("unpinned-two-nan-payloads", [K.QNAN, K.NAN_B]), ("unpinned-inf-minus-inf-then-nan", [K.PINF, K.NINF, K.QNAN])):
            x = row[name]
            assert x[~np.isfinite(x.view(F32))].tolist() == words, name      # bit patterns intact, in this order
        assert len(K.unpinned_rows(c)) == 4

    # channels: the per-row loader at >= 4096 rows, tiles that start mid-frame, a tile inside one frame, ragged
    fam = _family(cases, "channels")
    big = [c for c in fam if c.info["cls"] == "large"]
    assert [c.ch for c in big] == list(K.CHANNEL_COUNTS) and all(4096 <= c.M < 4096 + c.ch for c in big)
    assert all(256 % c.ch for c in big) and {c.ch for c in big if c.ch > 256} == {257, 300}
    assert sorted(c.ch for c in fam if c.info["cls"] == "small4") == [5, 33]
    assert all(c.src.n_samples % c.ch and c.f0 == 0 and c.f1 == c.src.n_frames for c in fam)

    # guards: tight shards in mid-stream, real PCM behind the partial last tile
    fam = _family(cases, "guards")
    assert {(c.ch, c.info["cls"] == "large") for c in fam} == {(2, False), (2, True), (3, False), (3, True)}
    for c in fam:
        _, t0, tc = c.shard()
        assert t0 == c.f0 * HOP - 512 and tc == (c.f1 - c.f0 - 1) * HOP + FRAME and c.f1 < c.src.n_frames
        assert c.M % 32 and c.M % 256 and c.info["halos"] == (0, 1, 3, 5)
        for h in c.info["halos"]:
            pcm, t0h, tch = c.shard(h)
            assert t0h == t0 - h and tch == tc + h and pcm.size == tch * c.ch

    # far: byte offsets of the first frame below / above 2^32, the last frames of each stream, ragged
    fam = _family(cases, "far")
    assert {c.src.n_samples for c in fam} == {(1 << 32) + 7, (1 << 33) + 12345, 3 * (1 << 33) + 5}
    assert {(c.ch, c.info["where"], k) for c in fam for k, _ in c.targets} >= \
        {(ch, wh, k) for ch in (2, 3) for wh in ("mid", "last") for k in ("small2", "small4", "sched", "dma", "st8", "st16")}
    for c in fam:
        assert c.src.n_samples % c.ch and c.src.data.size * 4 < 32 << 20      # a few MB stand for the stream
        first, last = c.f0 * HOP * c.ch * 4, (c.f1 - 1) * HOP * c.ch * 4
        if c.info["where"] == "mid":
            assert first < (1 << 32) < last and (1 << 32) - first < 1 << 25
        else:
            assert c.f1 == c.src.n_frames and first > 1 << 34
            assert c.shard()[0].size < c.shard()[2] * c.ch                    # the last sample frame is incomplete
    assert by["far-a-mid-large-3584"].ch == 2 and by["far-c-mid-large-4098"].ch == 3


def test_expected_outputs_hold_the_known_answers(cases, subsets):
    T, w, norm = O.tables()
    for c in _family(cases, "values"):
        rows, want = subsets[c.name]
        st = K.station_rows(c)
        at = {int(r): i for i, r in enumerate(rows)}
        for name in K.ZERO_STATIONS:                      # -0.0 and zero windows: every coefficient +0.0
            assert not bits(want[at[st[name]]]).any(), name
        for i in K.I_POS:                                 # an impulse reads out one table column times the window
            x = K.load_rows(c, [st[f"impulse-i{i}"]])[0, i]
            assert np.array_equal(bits(want[at[st[f"impulse-i{i}"]]]), bits(((x * w[i]) * T[:, i]) * norm)), i
        for name in ("subnormal-window", "subnormal-mixed", "tiny-at-ends"):
            assert np.isfinite(want[at[st[name]]]).all() and bits(want[at[st[name]]]).any()
        huge = want[at[st["huge"]]]
        assert np.isinf(huge).any() and np.isfinite(huge).any()                         # overflowed for some k only
        assert np.isinf(want[at[st["plus-inf"]]]).all() and np.isinf(want[at[st["minus-inf"]]]).all()
        both = want[at[st["inf-minus-inf"]]]
        assert np.isnan(both).any() and np.isinf(both).any()
        assert set(bits(both[np.isnan(both)]).tolist()) == {0xFFC00000}                  # inf - inf on x86
        for name in ("quiet-nan", "signalling-nan", "nan-then-inf-minus-inf"):          # the payload survives, quieted
            assert set(bits(want[at[st[name]]]).tolist()) == {K.QNAN}, name
        for r in K.unpinned_rows(c):
            assert np.isnan(want[at[r]]).all()


# which families are asked to notice which mutation (others may as well)
_HINT = {"fma": "all_rows", "two_accumulators": "all_rows", "descending_i": "all_rows", "neg_zero_init": "values",
         "subnormal_inputs_zero": "values", "subnormal_products_zero": "values", "norm_in_table": "all_rows",
         "window_in_table": "all_rows", "stages_swapped": "all_rows", "padding_reads_neighbour": "all_rows",
         "ragged_frame_dropped": "channels", "channel_off_by_one_above_256": "channels"}


_ANY_ROW = ("fma", "two_accumulators", "descending_i", "norm_in_table", "window_in_table", "stages_swapped")


def test_power_the_model_equals_the_oracle_and_every_mutation_shows(cases, subsets):
    """The numpy model gives the oracle's bits on the subset of every case (the unpinned rows aside, where it is
    numpy's operand order against gcc's), and every mutated copy of it changes an expected word in the family meant
    to catch it - which is what makes the GPU tests below able to catch such an edit of a kernel."""
    pinned = {}
    for c in cases:
        rows, want = subsets[c.name]
        pinned[c.name] = ~np.isin(rows, K.unpinned_rows(c))
        got = K.model(c, rows)
        assert rows[_differing_rows(got, want)].tolist() == K.unpinned_rows(c), c.name
    assert set(_HINT) == set(K.MUTATIONS) and len(K.MUTATIONS) == 12
    caught = {}
    for mut in K.MUTATIONS:
        fam = _family(cases, _HINT[mut])
        if mut in _ANY_ROW:
            fam = fam[:3] + fam[-1:]                       # any ordinary row shows these: four cases will do
        for c in fam:
            rows, want = subsets[c.name]
            p = pinned[c.name]
            hit = rows[p][_differing_rows(K.model(c, rows, mut)[p], want[p])]
            if hit.size:
                caught.setdefault(mut, {})[c.name] = hit.tolist()
    missed = [m for m in K.MUTATIONS if m not in caught]
    assert not missed, f"mutations no expected output notices: {missed}"
    print("mutation -> family that caught it (cases):",
          {m: (_HINT[m], len(v)) for m, v in caught.items()})
    by = _by_name(cases)
    # a sum that starts at -0.0 shows in one station only: where every product of a coefficient is -0.0
    for name, hit in caught["neg_zero_init"].items():
        assert hit == [K.station_rows(by[name])["zero-signed-against-column-0"]]
    assert set(caught["neg_zero_init"]) == {c.name for c in _family(cases, "values")}
    for mut in ("subnormal_inputs_zero", "subnormal_products_zero"):
        for name, hit in caught[mut].items():
            st = K.station_rows(by[name])
            assert {st["subnormal-window"], st["subnormal-mixed"]} <= set(hit) if mut == "subnormal_inputs_zero" else st["tiny-at-ends"] in hit
    assert set(caught["channel_off_by_one_above_256"]) == {c.name for c in _family(cases, "channels") if c.ch > 256}
    assert set(caught["ragged_frame_dropped"]) == {c.name for c in _family(cases, "channels")}
    for name, hit in caught["ragged_frame_dropped"].items():
        assert by[name].M - by[name].ch in hit             # channel 0 of the last frame holds the odd sample
    for mut in _ANY_ROW:
        assert len(caught[mut]) == 4, mut
    # leading padding is read by frame 0, trailing padding by the last frames: both ends show a wrong padding rule
    assert "all-ch1-small2-1" in caught["padding_reads_neighbour"] and 0 in caught["padding_reads_neighbour"]["all-ch1-large-4097"]
    assert 4096 in caught["padding_reads_neighbour"]["all-ch1-large-4097"]


# ----------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------

PAD_ROWS = 256          # sentinel rows in front of and behind every coefficient destination
PCM_PAD = 16384         # NaN floats (64 KiB) in front of and behind every shard


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    import glc_amd
    f = glc_amd.lib.glc_debug_set_mdct_variant
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int]
    return torch, glc_amd


def _device_shard(torch, case, halo):
    """The shard on the device with NaN on both sides -> (tensor, address of the shard, t0, t_count)."""
    pcm, t0, tc = case.shard(halo)
    host = np.full(pcm.size + 2 * PCM_PAD, K.POISON_BITS, np.uint32)
    host[PCM_PAD:PCM_PAD + pcm.size] = pcm.view(np.uint32)       # as words: a signalling NaN travels untouched
    d = torch.from_numpy(host.view(np.int32)).cuda()
    return d, d.data_ptr() + 4 * PCM_PAD, t0, tc


def _explain(got, exp):
    bad = np.argwhere(got != exp)
    rows = np.unique(bad[:, 0])
    r, k = bad[0]
    return (f"{len(bad)} words differ ({int((got[got != exp] == K.SENTINEL_BITS).sum())} never written) in {rows.size} rows; first: row {r} "
            f"k {k}, got {got[r, k]:#010x} want {exp[r, k]:#010x}; rows {rows[:12].tolist()}")


def _check_destination(buf, M, what):
    """buf: the whole destination buffer as words -> the M rows between the sentinel rows, those intact."""
    buf = buf.reshape(-1, HOP)
    front, back = buf[:PAD_ROWS], buf[PAD_ROWS + M:]
    assert (front == K.SENTINEL_BITS).all(), f"{what}: words in front of the destination were written"
    assert (back == K.SENTINEL_BITS).all(), \
        f"{what}: rows behind the destination were written: {(np.flatnonzero((back != K.SENTINEL_BITS).any(axis=1)) + M)[:8].tolist()}"
    return buf[PAD_ROWS:PAD_ROWS + M]


def _forward(gpu, enc, case, variant, halo=0, records=False):
    """One launch of frames [f0, f1) with `variant` pinned -> coefficient words [M, 1024] (and the record bytes when
    the launch goes through glc_encode_range_device with a coefficient tap)."""
    torch, glc_amd = gpu
    what = f"{case.name} variant {variant} halo {halo}"
    keep, p_pcm, t0, tc = _device_shard(torch, case, halo)
    d = torch.full(((case.M + 2 * PAD_ROWS) * HOP,), K.SENTINEL_BITS, dtype=torch.int32, device="cuda")
    p_coef = d.data_ptr() + 4 * PAD_ROWS * HOP
    rb = glc_amd.lib.glc_record_bytes(case.ch) * (case.f1 - case.f0)
    d_rec = None
    if records:     # zeroed, as the oracle's are: the header padding and the upper half of a compressed row are nobody's
        d_rec = torch.full((rb + 8192,), 0xA5, dtype=torch.uint8, device="cuda")
        d_rec[4096:4096 + rb] = 0
    torch.cuda.synchronize()
    assert glc_amd.lib.glc_debug_set_mdct_variant(enc._h, variant) == 0
    try:
        if records:
            enc.encode_range_device(p_pcm, t0, tc, case.src.n_samples, case.ch, case.f0, case.f1, d_rec.data_ptr() + 4096, p_coef)
        else:
            enc.mdct_forward_device(p_pcm, t0, tc, case.src.n_samples, case.ch, case.f0, case.f1, p_coef)
        enc.synchronize()
    finally:
        assert glc_amd.lib.glc_debug_set_mdct_variant(enc._h, 0) == 0
    coef = _check_destination(d.cpu().numpy().view(np.uint32), case.M, what)
    del keep
    if not records:
        return coef
    r = d_rec.cpu().numpy()
    assert (r[:4096] == 0xA5).all() and (r[4096 + rb:] == 0xA5).all(), f"{what}: bytes around the records were written"
    return coef, r[4096:4096 + rb]


def _case_ids(*families):
    return [c.name for c in K.cases() if c.family in families]


@pytest.mark.gpu
@pytest.mark.parametrize("name", _case_ids("values", "all_rows", "channels", "guards", "far"))
def test_gpu_every_row_of_every_case_on_every_kernel(gpu, cases, name):
    """All rows against the oracle, bit for bit, NaN bits included.  The unpinned rows: NaN where the oracle has
    NaN, the same words from every kernel that can run this row count - and, as it turned out, the C oracle's."""
    c = _by_name(cases)[name]
    exp = bits(K.expected(c))
    un = K.unpinned_rows(c)
    pinned = np.ones(c.M, bool)
    pinned[un] = False
    enc = gpu[1].Encoder(c.src.sr)
    words = {}
    for kernel, variant in c.targets:
        assert K.kernel_for(c.M, c.ch, variant) == kernel
        got = _forward(gpu, enc, c, variant)
        assert np.array_equal(got[pinned], exp[pinned]), f"{name} on {kernel}: {_explain(got[pinned], exp[pinned])}"
        if un:
            nan = (exp[un] & 0x7FFFFFFF) > 0x7F800000
            assert nan.all() and np.array_equal((got[un] & 0x7FFFFFFF) > 0x7F800000, nan), f"{name} on {kernel}: NaN positions"
            words[kernel] = got[un].copy()
    first = next(iter(words.values()), None)
    for kernel, w in words.items():
        assert np.array_equal(w, first), f"{name}: {kernel} and {next(iter(words))} give different words in the unpinned rows"
    if un:      # measured on the MI355X, a property of the shipped kernels and not of the reference:
        # the running sum is the add's first source in all six, and its NaN is the one handed on - gcc's choice too
        assert np.array_equal(first, exp[un]), f"{name}: the unpinned rows no longer hold the C oracle's words"


@pytest.mark.gpu
@pytest.mark.parametrize("name", _case_ids("guards"))
def test_gpu_guards_extra_halo_nan_around_the_shard_sentinels_around_the_destination(gpu, cases, name):
    """A tight shard and one with 1 / 3 / 5 samples more in front (a source base that is not the first window's
    first sample, odd element offsets): nothing outside the legal span reaches a coefficient (all finite, all
    equal to the oracle), no row at or behind M of the partial last tile is stored."""
    c = _by_name(cases)[name]
    exp = bits(K.expected(c))
    assert np.isfinite(exp.view(F32)).all()
    enc = gpu[1].Encoder(c.src.sr)
    for halo in c.info["halos"]:
        for kernel, variant in c.targets:
            got = _forward(gpu, enc, c, variant, halo)
            assert np.isfinite(got.view(F32)).all(), f"{name} on {kernel}, halo {halo}: a sample outside the shard reached a coefficient"
            assert np.array_equal(got, exp), f"{name} on {kernel}, halo {halo}: {_explain(got, exp)}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", _case_ids("far"))
def test_gpu_far_offsets_through_the_encode_range(gpu, cases, name):
    """The far shards through glc_encode_range_device: K1 by the same dispatch, then K2 and (3 channels) K3 with
    their own 64-bit offsets into the PCM for the raw plane - coefficient words and record bytes."""
    c = _by_name(cases)[name]
    co, rec, is_raw = K.expected(c, records=True)
    assert is_raw.any() and not is_raw.all()             # raw planes and quantised rows
    enc = gpu[1].Encoder(c.src.sr)
    for kernel, variant in c.targets:
        got, got_rec = _forward(gpu, enc, c, variant, records=True)
        assert np.array_equal(got, bits(co)), f"{name} on {kernel}: {_explain(got, bits(co))}"
        bad = np.flatnonzero(got_rec != rec)
        assert bad.size == 0, f"{name} on {kernel}: {bad.size} record bytes differ, first at {bad[0]} (record of {O.record_bytes(c.ch)} bytes)"
