"""Cases and models for tests/test_encode_screen_edges.py: the screened encode path at the edges
tests/encode_screen_cases.py does not reach - the channel counts of every loader and of both quantiser forms, failing
rows on either side of the 4 / 16 / 32 / 256-row cuts of its three stages, energy confined to one octet of bound
columns or to the exact bins just below C0, one workspace used by launches of changing size and channel count, and
the four drivers besides glc_encode_range_device.

Two models, neither of them the code under test:
  conditions() / encode_screen_cases.model()   which rows pass, from the oracle's coefficients;
  screen_records()                             the RECORDS the three stages leave, from the oracle's coefficients and
                                               its quantiser, with the stages' row cuts (waves of 4, groups of 16,
                                               tiles of 32) written out - and, on request, with one of MUTATIONS
                                               applied, which is how the suite shows that a wrong cut would be seen."""
import numpy as np

import encode_screen_cases as S
from encode_screen_cases import (C_ERR, F32, FRAME, HOP, NOISE_FLOOR, SLACK, TINY, Case, _click, expected,  # noqa: F401
                                 lcg_noise, model, shape, tones, windowed_rows)
from oracle import oracle as O

SR = 48000
# tones below the last band at every channel count: tones() spreads by 1 + 0.013 c, 16 channels put 5200 Hz at 6214
LOW = ([220.0, 1234.5, 3100.0, 5200.0], [0.3, 0.2, 0.1, 0.05])
RATES = (44100, 48000, 96000, 192000)


class Edge(Case):
    """A range case that knows which rows it was built to fail: `fail_rows` exactly (None: `must_fail` at least,
    `must_pass` never - the octet cases whose stretch ends fade)."""

    def __init__(self, name, family, sr, ch, pcm, f0, f1, fail_rows=None, must_fail=(), must_pass=(), **tags):
        super().__init__(name, family, sr, ch, pcm, f0, f1)
        self.fail_rows = None if fail_rows is None else sorted(set(int(r) for r in fail_rows))
        self.must_fail, self.must_pass = sorted(set(must_fail)), sorted(set(must_pass))
        self.tags = tags


def stream(sr, ch, frames):
    return tones(sr, ch, frames * HOP, *LOW)


def guarded_shard_case(ch=2):
    """258 rows from frame 5 of a longer stream - one 256-row tile of the FMA form of the transform and one frame
    more, two 128-row tiles of the matrix form and one frame more - with a click in one frame, so that a few rows fail
    and the repair runs.  Its tight shard starts inside the stream (t0 > 0) and ends inside it; the GPU test puts NaN
    on both sides of it, so a descriptor that reached one sample too far on either side would show in the records.
    ch = 2: the segment loader; ch = 3: one dword per (row, sample), tiles that start inside a frame."""
    assert 258 % ch == 0
    f0, nf = 5, 258 // ch
    x = stream(SR, ch, f0 + nf + 4)
    _click(x, f0 + nf // 2)
    return Case(f"guarded-shard-ch{ch}", "guarded", SR, ch, x, f0, f0 + nf)


# ---------------------------------------------------------------------------------------------------- 1: channels

def channel_cases():
    """Every loader (4, 8 and the generic one at 5 / 6 / 16) and both quantiser forms: a click in the first, the last
    and a middle channel alone, one in all channels; noise at 4 and 8 channels, compressed and raw."""
    out = []
    for ch, nf in ((4, 70), (5, 53), (6, 45), (8, 35), (16, 20)):      # 280, 265, 270, 280, 320 rows
        f0 = 3
        x = stream(SR, ch, f0 + nf + 3)
        rows = []
        for i, c in enumerate((0, ch - 1, ch // 2, None)):
            f = (i + 1) * nf // 5
            _click(x, f0 + f, ch_sel=c)
            hit = range(ch) if c is None or ch == 4 else [c]          # fused (4): the frame; otherwise the row
            rows += [f * ch + q for q in hit]
        out.append(Edge(f"ch{ch}-clicks", "channels", SR, ch, x, f0, f0 + nf, fail_rows=rows, values="click"))
    for ch, nf in ((4, 66), (8, 33)):                                 # 264 rows
        n = (nf + 2) * HOP
        quiet = lcg_noise(n, ch, seed=99, amp=0.05) + tones(SR, ch, n, [440.0], [0.5])
        out.append(Edge(f"ch{ch}-noise", "channels", SR, ch, quiet, 1, 1 + nf, fail_rows=range(nf * ch), raw=False))
        out.append(Edge(f"ch{ch}-noise-raw", "channels", SR, ch, lcg_noise(n, ch), 1, 1 + nf, fail_rows=range(nf * ch), raw=True))
    return out


# ---------------------------------------------------------------------------------------------------- 2: boundaries

M_MONO = 256 + 32 + 16 + 4 + 1       # a full tile, then a partial one that ends in a partial 32-tile, 16-group and wave
M_STEREO = M_MONO + 1
CUTS = (4, 16, 32, 256)


def boundary_patterns(M):
    """name -> failing ROWS of a mono launch of M rows (a stereo launch fails the frames that hold them)."""
    first_of_last = (M - 1) // 32 * 32
    singles = [0] + [r for c in CUTS for r in (c - 1, c)] + [M - 1, first_of_last]
    pat = {f"r{r}": [r] for r in singles}
    pat["all-cuts"] = singles
    pat["tile1-fails"] = list(range(32, 64))
    pat["tile1-passes"] = list(range(0, 32)) + list(range(64, 96))
    return pat


def boundary_cases():
    out = []
    for ch, M in ((1, M_MONO), (2, M_STEREO)):
        nf, f0 = M // ch, 3
        base = stream(SR, ch, f0 + nf + 3)
        pats = {k: sorted({r // ch for r in v}) for k, v in boundary_patterns(M).items()}
        pats["alternate"] = list(range(0, nf, 2))
        for tag, frames in pats.items():
            x = base.copy()
            for f in frames:
                _click(x, f0 + f)
            out.append(Edge(f"b{ch}-{tag}", "boundaries", SR, ch, x, f0, f0 + nf,
                            fail_rows=[f * ch + c for f in frames for c in range(ch)]))
    return out


# ---------------------------------------------------------------------------------------------------- 3: octets

def line_stream(sr, k, over_floor_db, frames):
    """A tone at the centre of bin kt (about 1 kHz) in a phase that gives every frame the same scale, and, in hops
    8..15, 24..31, ... only, a line at the centre of bin k whose coefficient in the EVEN frames (the phase turns a
    quarter per frame) stands `over_floor_db` above the noise floor, alone but for bins k +- 2 at -23.5 dB; the odd
    frames hold it as bins k +- 1 at -6.6 dB each."""
    n = frames * HOP
    t = np.arange(n, dtype=np.float64)
    kt = int(round(1000.0 * 2048 / sr - 0.5))
    at = 0.5

    def at_bin(kk, theta0):
        w = np.pi * (kk + 0.5) / HOP
        return np.cos(w * (t + 1024.5) + theta0)
    al = at * np.cos(np.pi / 4) * float(NOISE_FLOOR) * 10.0 ** (over_floor_db / 20.0)
    on = (np.arange(n) // HOP // 8) % 2 == 1
    return (at * at_bin(kt, np.pi / 4) + on * al * at_bin(k, 0.0))[:, None]


LOUD, CONFINED, LONE = 31.0, 14.0, 3.0     # dB over the floor: "about -20 dB" under the tone; one octet; one bin
# ... and half a dB UNDER it: nothing of the row is over the floor, and the row fails all the same, because the
# bound adds kScreenCErr A to the fused sums - 0.944 nfl without it, 1.055 nfl with it.  Only A fails these rows.
SUBFLOOR = -0.5


def octet_cases():
    out = []
    f0, nf = 2, 260
    for sr in RATES:
        L, c0, _ = shape(sr)
        ks = [(c0, LOUD), (1022, LOUD)]
        if sr <= 48000:
            ks += [(c0 + 7, LOUD), (c0 + 8, LOUD), (1015, LOUD), (1016, LOUD), (c0 + 3, CONFINED), (1020, CONFINED),
                   (L, LONE), (c0 - 1, LONE)]
        ks += {44100: [(c0 + 3, SUBFLOOR)], 48000: [(1020, SUBFLOOR)]}.get(sr, [])
        for k, db in ks:
            x = line_stream(sr, k, db, f0 + nf + 4)
            stretch = [f for f in range(f0, f0 + nf) if (f // 8) % 2 == 1]           # frames that hold the line throughout
            edge = {f for f in range(f0, f0 + nf) if (f // 8) % 2 == 0 and f % 8 in (0, 7)}   # ... and for 512 samples
            off = [f for f in range(f0, f0 + nf) if (f // 8) % 2 == 0 and f not in edge]
            whole = [f for f in stretch if f % 8 not in (0, 7)]
            kw = dict(k=k, db=db, values="line")
            if db == LOUD:      # the stretch and the frame on either side, whose window holds 512 samples of the line
                kw["fail_rows"] = [f - f0 for f in stretch] + [f - f0 for f in edge]
            elif db == CONFINED:
                kw["must_fail"], kw["must_pass"] = [f - f0 for f in whole], [f - f0 for f in off]
            elif db == SUBFLOOR:    # the even frames that hold the line throughout; the fused sums decide (decide())
                kw["fail_rows"], kw["decide"] = [f - f0 for f in whole if f % 2 == 0], "fma"
            else:               # one bin, 3 dB over the floor in the even frames; 3.6 dB under it, twice, in the odd ones
                kw["must_fail"] = [f - f0 for f in whole if f % 2 == 0]
                kw["must_pass"] = [f - f0 for f in off] + [f - f0 for f in whole if f % 2 == 1]
            out.append(Edge(f"{'sub' if db == SUBFLOOR else 'oct'}-{sr}-k{k}", "octets", sr, 1, x, f0, f0 + nf, **kw))
    return out


# ---------------------------------------------------------------------------------------------------- 4: reuse

def reuse_cases():
    out = []
    x = np.tile(lcg_noise(130 * HOP, 2), (3, 1))
    out.append(Edge("reuse-fail-768", "reuse", SR, 2, x, 1, 385, fail_rows=range(768)))
    out.append(Edge("reuse-pass-290", "reuse", SR, 2, stream(SR, 2, 153), 4, 149, fail_rows=[]))
    x = stream(SR, 1, 310)
    for f in (0, 150, 300):
        _click(x, 3 + f)
    out.append(Edge("reuse-mixed-301", "reuse", SR, 1, x, 3, 304, fail_rows=[0, 150, 300]))
    x = stream(SR, 3, 110)
    _click(x, 3 + 40, ch_sel=1)
    _click(x, 3 + 99)
    out.append(Edge("reuse-ch3", "reuse", SR, 3, x, 3, 103, fail_rows=[40 * 3 + 1, 297, 298, 299]))
    x = stream(SR, 1, 265)
    _click(x, 3 + 254)
    _click(x, 3 + 255)
    out.append(Edge("reuse-m255", "reuse", SR, 1, x, 3, 258, fail_rows=[254]))
    out.append(Edge("reuse-m256", "reuse", SR, 1, x, 3, 259, fail_rows=[254, 255]))
    return out


# the sequences, each on the ONE context the reuse tests share, in this order
SEQUENCES = {
    "shrink": ["reuse-fail-768", "reuse-pass-290", "reuse-mixed-301"],
    "channels": ["b2-all-cuts", "ch8-clicks", "reuse-ch3", "b2-alternate"],
    "twice": ["reuse-mixed-301", "reuse-mixed-301"],
    "threshold": ["reuse-m255", "reuse-m256"],
}


def range_cases():
    return channel_cases() + boundary_cases() + octet_cases()


def all_cases():
    return range_cases() + reuse_cases()


# ---------------------------------------------------------------------------------------------------- 5: drivers

def encode_rounds(n_frames, ch):
    """The rounds of glc_encode: pieces of 2048 / ch frames while the stream opens, no round for
    less than half a piece -> [(f0, nf)].  (A stream of these sizes never reaches the full-size rounds.)"""
    piece = max(1, 2048 // ch)
    out, f = [], 0
    while f < n_frames:
        assert f < 4 * piece
        nf = min(piece, n_frames - f)
        if n_frames - f - nf < piece // 2:
            nf = n_frames - f
        out.append((f, nf))
        f += nf
    return out


ENCODE_CH, ENCODE_FRAMES = 8, 690
ENCODE_CLICKS, ENCODE_NOISE = (100, 600), (300, 340)        # frames: rounds 0 and 2; inside round 1 (workspace slot 1)


def encode_clip():
    """690 frames of 8 channels: rounds of 256, 256 and 178 frames."""
    ch, nf = ENCODE_CH, ENCODE_FRAMES
    x = stream(SR, ch, nf)[:nf * HOP - 300]
    for f in ENCODE_CLICKS:
        _click(x, f, ch_sel=5)
    a, b = ENCODE_NOISE
    x[a * HOP:b * HOP] += lcg_noise((b - a) * HOP, ch, seed=7, amp=0.3)
    return np.ascontiguousarray(x, F32)


def encode_clip_i16():
    """encode_clip() as 16-bit integers [n, ch]."""
    return np.clip(np.rint(encode_clip().astype(np.float64) * 32767.0), -32768, 32767).astype(np.int16)


def whole_case(name, sr, ch, x):
    """The whole stream `x` [n, ch] as a Case."""
    x = np.ascontiguousarray(x, F32)
    return Case(name, "drivers", sr, ch, x, 0, O.num_frames(x.size, ch))


def virtual_stream(clips, ch):
    """The stream a batch driver launches: clip i of nf_i frames owns (nf_i + 1) * 1024 samples
    per channel, its own at the front and zeros behind them; frame nf_i of its slot is junk.
    -> (samples [V * 1024, ch], [(first virtual frame, nf_i)])."""
    nfs = [O.num_frames(c.size, ch) for c in clips]
    V = sum(nfs) + len(clips)
    vs = np.zeros((V * HOP, ch), F32)
    at, slots = 0, []
    for c, nf in zip(clips, nfs):
        vs[at * HOP:at * HOP + c.size // ch] = c.reshape(-1, ch)
        slots.append((at, nf))
        at += nf + 1
    return vs, slots


def virtual_case(name, sr, ch, clips):
    vs, slots = virtual_stream(clips, ch)
    c = Case(name, "drivers", sr, ch, vs, 0, vs.shape[0] // HOP)
    c.slots = slots
    return c


def batch_clips(sr, ch, n, frames, seed=1):
    """n clips of `frames[i % len]` frames, their content in turn: tonal, LCG noise, silence, a click in the first
    frame, a click in the last."""
    out = []
    for i in range(n):
        nf = frames[i % len(frames)]
        ln = nf * HOP + 400 - 37 * (i % 5)                 # (nf frames: 512 + ln rounds up to nf + 1 hops)
        kind = i % 5
        if kind == 1:
            x = lcg_noise(ln, ch, seed=seed + i)
        elif kind == 2:
            x = np.zeros((ln, ch))
        else:
            x = tones(sr, ch, ln, *LOW, phase=0.3 + 0.1 * i)
            if kind == 3:
                x[512, :] += 2.0
            if kind == 4:
                x[(nf - 1) * HOP + 512, :] += 2.0
        x = np.ascontiguousarray(x, F32).reshape(-1)
        assert O.num_frames(x.size, ch) == nf
        out.append(x)
    return out


def encode_batch_clips():
    return batch_clips(SR, 2, 20, (5, 6, 7, 8, 9))          # V = 160 virtual frames, 320 rows


def roundtrip_batches():
    """(name, sr, ch, planar, clips): a planar stereo batch (V = 139, 278 rows) and an interleaved one of 3 channels
    (V = 95, 285 rows)."""
    return [("rt-planar-ch2", SR, 2, True, batch_clips(SR, 2, 14, (8, 9, 10), seed=31)),
            ("rt-interleaved-ch3", SR, 3, False, batch_clips(SR, 3, 10, (8, 9), seed=57))]


def roundtrip_clip():
    x = stream(SR, 2, 150)[:150 * HOP - 700]
    _click(x, 70)
    return np.ascontiguousarray(x, F32).reshape(-1)


# ---------------------------------------------------------------------------------------------------- the decision

MUTATIONS = {
    1: "hf and A taken from row m + 1",
    2: "the first octet ignored",
    3: "the last octet ignored",
    4: "A dropped from the bound",
    5: "condition (a) from k > l0",
    6: "condition (a) stops at c0 - 1",
    7: "repair flags read from the previous 32-tile",
    8: "the partial last 32-tile never repaired",
    9: "MODE 2's 16-row ballot shifted by one group",
    10: "flags of a larger launch kept for rows >= M",
    11: "a fused frame not failed by its sibling",
}


_fused = {}


def fused(case):
    """(|e_k| of the columns C0.., A) of every row as the bound waves form them: the float32 emulation of the fused
    sums (encode_screen_cases.fma_sums) and the ascending float32 sum of |x w|.  Kept per case."""
    if case.name not in _fused:
        T, _, _ = O.tables()
        xw = windowed_rows(case)
        e = S.fma_sums(xw, T, np.arange(shape(case.sr)[1], HOP))
        _fused[case.name] = (np.abs(e), np.cumsum(np.abs(xw), axis=1, dtype=F32)[:, -1])
    return _fused[case.name]


def conditions(case, taps, mut=None, ratio=False):
    """-> (a, b): per row whether condition (a) - an exact bin of [L, C0) over the floor - and condition (b) - the
    bound of the columns >= C0 over the floor, or not finite - fail it.  The bound is formed from the oracle's own
    coefficients in place of the fused sums: right wherever model() decides a row, which most cases are built for.
    A case tagged decide="fma" sits where model() cannot decide - inside the bracket 2 gamma_2048 A it allows the
    fused sums - so its bound is formed from their emulation, fused().  ratio: -> B / nfl instead of b."""
    L, c0, _ = shape(case.sr)
    _, _, norm = O.tables()
    a = np.abs(taps.coeffs.astype(np.float64))
    nfl = float(NOISE_FLOOR) * np.maximum(a[:, :c0].max(1), 1e-10)
    lo, hi = (L + 1 if mut == 5 else L), (c0 - 1 if mut == 6 else c0)
    cond_a = (a[:, lo:hi] > nfl[:, None]).any(1)
    if getattr(case, "tags", {}).get("decide") == "fma":
        e, A = fused(case)
        e, A = e.astype(np.float64), A.astype(np.float64)
    else:
        e, A = a[:, c0:] / float(norm), np.abs(windowed_rows(case).astype(np.float64)).sum(1)
    first, last = (8 if mut == 2 else 0), (HOP - c0 - 8 if mut == 3 else HOP - c0)
    hs = e[:, first:last].max(1)
    if mut == 1:        # the planes are padded with zeros behind row M - 1
        hs, A = np.append(hs[1:], 0.0), np.append(A[1:], 0.0)
    if mut == 4:
        A = np.zeros_like(A)
    B = (hs + float(C_ERR) * A) * float(norm) * float(SLACK) + float(TINY)
    return cond_a, (B / nfl if ratio else ~(B <= nfl))


def decide(case, taps):
    """model() of a case - or, for a case tagged decide="fma", the decision of the emulated fused sums: +1 / -1 per
    row (the CPU tests assert the margin that makes it a decision)."""
    if getattr(case, "tags", {}).get("decide") != "fma":
        return model(case, taps)
    a, b = conditions(case, taps)
    return np.where(a | b, -1, 1)


def flags(case, taps, mut=None):
    """Per row what MODE 1 leaves in row_flag."""
    a, b = conditions(case, taps, mut)
    fail = a | b
    if case.ch in (1, 2, 4) and mut != 11:
        fail = np.repeat(fail.reshape(-1, case.ch).any(1), case.ch)
    return fail


# ---------------------------------------------------------------------------------------------------- the records

class Rows:
    """Per row of a case what each stage can write: the oracle's row, the MODE 1 row (columns >= C0 count as zero,
    the last band's base is 0) and the MODE 0 row of coefficients whose columns >= C0 were never computed (a
    workspace that holds zeros there).  Computed on demand, kept."""

    def __init__(self, case, taps):
        self.case, self.taps = case, taps
        self.L, self.c0, _ = shape(case.sr)
        self.weights, self.edges = O.perceptual(case.sr)
        self._pass, self._blind = {}, {}

    def exact(self, m):
        return self.taps.scales[m], int(self.taps.nnz[m]), self.taps.dense_q[m]

    def _quant(self, m, last_base_zero):
        c = self.taps.coeffs[m].copy()
        c[self.c0:] = 0
        scale = np.maximum(np.abs(c).max(), F32(1e-10))
        thr = O.thresholds(c, self.weights, self.edges)
        if last_base_zero:
            thr[self.L:] = 0
        idx, q = O.compress(c, scale, thr)
        dense = np.zeros(HOP, np.int16)
        dense[idx] = q
        return F32(scale), int(idx.size), dense

    def passing(self, m):
        if m not in self._pass:
            self._pass[m] = self._quant(m, True)
        return self._pass[m]

    def blind(self, m):
        if m not in self._blind:
            self._blind[m] = self._quant(m, False)
        return self._blind[m]


def screen_records(case, rows, exp_rec, fail, mut=None, stale=None):
    """The records the screened path leaves in a zeroed buffer when MODE 1 flags the rows `fail`:
    -> (record bytes, rows counted as repaired, rows >= M that a stage would write)."""
    M, ch = case.M, case.ch
    fail = np.asarray(fail, bool)
    flag = np.zeros((M + 31) // 32 * 32 + 32, bool)          # what a stage finds in row_flag; nothing is set behind M ...
    if mut == 10 and stale is not None:                       # ... unless a stage forgets to stop at M
        n = min(flag.size, stale.size)
        flag[:n] = stale[:n]
    flag[:M] = fail
    n32 = (M + 31) // 32
    tile_on = np.array([flag[(t - 1) * 32:t * 32].any() if mut == 7 else flag[t * 32:t * 32 + 32].any() for t in range(n32)])
    if mut == 7:
        tile_on[0] = False
    if mut == 8 and M % 32:
        tile_on[-1] = False
    shift = 16 if mut == 9 else 0
    n16 = (M + 15) // 16
    on2 = np.zeros(n16 * 16, bool)                            # rows MODE 2 writes
    for g in range(n16):
        on2[g * 16:g * 16 + 16] = flag[g * 16 + shift:g * 16 + 16 + shift]
    stray = [int(r) for r in np.flatnonzero(on2) if r >= M]
    on2 = on2[:M]
    rec_b = O.record_bytes(ch)
    hdr = (8 + 8 * ch + 15) // 16 * 16
    out = np.zeros((M // ch, rec_b), np.uint8)
    exp = exp_rec.reshape(M // ch, rec_b)
    raw_limit = F32(2 * FRAME * ch) * F32(0.85)
    for f in range(M // ch):
        got = []
        for c in range(ch):
            m = f * ch + c
            if on2[m]:
                got.append(rows.exact(m) if tile_on[m // 32] else rows.blind(m))
            elif not fail[m]:
                got.append(rows.passing(m))
            else:
                got.append(None)                              # failed and never repaired: nobody writes it
        if all(g is None for g in got):
            continue
        r = out[f]
        compressed = 8 + 4 * ch + 64 + sum(8 + 4 * (g[1] if g else 0) for g in got)
        raw = F32(compressed) >= raw_limit
        r[:4] = np.frombuffer(np.uint32(raw).tobytes(), np.uint8)
        for c, g in enumerate(got):
            if g is None:
                continue
            r[8 + 8 * c:12 + 8 * c] = np.frombuffer(F32(g[0]).tobytes(), np.uint8)
            r[12 + 8 * c:16 + 8 * c] = np.frombuffer(np.uint32(g[1]).tobytes(), np.uint8)
            at = hdr + c * 2 * FRAME
            if raw:                                           # the windowed plane does not depend on a coefficient
                assert exp[f, 0] == 1, "a frame the oracle compresses went raw: not modelled"
                r[at:at + 2 * FRAME] = exp[f, at:at + 2 * FRAME]
            else:
                r[at:at + 2 * HOP] = np.frombuffer(g[2].tobytes(), np.uint8)
    return out.reshape(-1), int(fail.sum()), stray
