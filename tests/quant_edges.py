"""Deterministic coefficient rows that sit on the quantiser's decision edges, and the frame records the
device path must write for them (test helper, numpy + the CPU oracle only).

K2 (k_quantize) and K3 (k_decide_raw) branch on data: a per-bin masking threshold, a noise floor, a peak
gate, round half away from zero, an i16 clamp, and a raw-or-compressed decision at a byte count
(src/codec.rs:188-240, :270-311, :496-521).  Coefficients that come out of the forward transform of real
audio almost never sit within an ulp of one of those edges, so the parity suite cannot tell a kernel
that computes them one rounding differently.  The families built here can:

  thresholds  one bin per band and row bisected (f32 bit pattern) until two adjacent floats straddle the
              keep / drop decision; the rows hold one side or the other (both sides across rows), at the
              sample rates of RATES, which between them take every body-loop step count of K2's phase 2
  noise_floor |c| == f32(10^(-48/20) * scale) (dropped) and the next float up (kept)
  peak_gate   |c| == f32(scale * 0.3) (not a peak, dropped) and the next float up (a peak, kept)
  rounding    scale 1: c = +-(k + 0.5) / 32768 -> +-(k + 1), the floats beside them, +-scale, clamps
  extremes    zero, subnormal, repeated negative maximum, overflowing band energy, NaN and inf rows
  raw         total nnz per frame at the raw-or-compressed flip point - 1, + 0, + 1 for 1..8 and 16
              channels, PCM with values past +-1, +-inf and NaN, a frame range and shard that start late

`Case.expected` comes from the C oracle (scale, thresholds, q per row) and from a numpy f32 restatement
of src/codec.rs:496-521 (decision, raw plane); `quantise` / `decide` restate the quantiser in numpy with
optional mutations, which tests/test_quantizer_edges.py uses to show that the families would notice an
edit of the arithmetic.
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle as O

F32 = np.float32
HOP, FRAME = 1024, 2048
SENTINEL = 0xA5
NOISE_FLOOR = F32(0.003981071058660746)  # 10f32.powf(-48 / 20), bits 0x3b8273a5
RATES = (100, 1000, 1500, 2000, 2500, 4500, 8000, 11025, 12345, 16000, 22050, 44100, 48000, 96000, 192000)
# the phase-2 body-loop step counts the RATES take between them (test_quantizer_edges asserts this set)
BODY_STEPS = {0, 1, 2, 3, 4, 5, 6, 7, 8, 17, 40, 42, 53, 57, 64}
CHANNELS = (1, 2, 3, 4, 5, 6, 7, 8, 16)
ODD_RATE = 12345

MUTATIONS = ("thr_ulp_up", "thr_ulp_down", "sum_two_acc", "sum_descending", "ge_threshold", "ge_noise_floor",
             "ge_peak", "ties_even", "gt_raw", "fold_base_constant")


def record_bytes(ch: int) -> int:
    return O.record_bytes(ch)


def header_bytes(ch: int) -> int:
    return ((8 + 8 * ch) + 15) // 16 * 16


def body_steps(lo: int, hi: int) -> int:
    """Steps of K2's 16-bin body loop for band [lo, hi): head to 4-alignment first (glc_kernels.hip phase 2)."""
    i = lo
    while i < hi and i & 3:
        i += 1
    return (hi - i) // 16 if i + 16 <= hi else 0


# ----------------------------------------------------------------------------------------------------
# numpy restatement of src/codec.rs:188-240 + :270-311 + :505-521, with optional mutations
# ----------------------------------------------------------------------------------------------------

_perceptual_cache: dict = {}


def perceptual(sr: int):
    if sr not in _perceptual_cache:
        _perceptual_cache[sr] = O.perceptual(sr)
    return _perceptual_cache[sr]


def _band_sum(sq: np.ndarray, mut) -> np.ndarray:
    """Sum of squares of one band per row: ascending, one accumulator (src/codec.rs:212-214)."""
    n = sq.shape[1]
    if mut == "sum_two_acc":
        a, b = np.zeros(sq.shape[0], F32), np.zeros(sq.shape[0], F32)
        for i in range(0, n, 2):
            a = a + sq[:, i]
            if i + 1 < n:
                b = b + sq[:, i + 1]
        return a + b
    ss = np.zeros(sq.shape[0], F32)
    order = range(n - 1, -1, -1) if mut == "sum_descending" else range(n)
    for i in order:
        ss = ss + sq[:, i]
    return ss


def band_thresholds(vals: np.ndarray, wts: np.ndarray, gmax: np.ndarray, mut=None) -> np.ndarray:
    """thresholds[i] of one band (vals [R, len], its weights, the rows' global max): src/codec.rs:211-236."""
    ln = F32(vals.shape[1])
    ss = _band_sum(vals * vals, mut)
    energy = np.sqrt(ss / ln)
    ws = F32(0.0)
    for x in wts:
        ws = F32(ws + x)
    avg = F32(ws / ln)
    cf = max(F32(1.0) - F32(0.7), F32(0.01))
    pf = F32(1.0) / max(avg, F32(0.1))
    if mut == "fold_base_constant":
        base = energy * F32(F32(F32(0.01) * cf) * pf)
    else:
        base = ((energy * F32(0.01)) * cf) * pf
    indiv = (F32(1.0) / np.maximum(wts, F32(0.1))).astype(F32)
    t = base[:, None] * indiv[None, :]
    a, gate = np.abs(vals), (gmax * F32(0.3))[:, None]
    peak = a >= gate if mut == "ge_peak" else a > gate
    t = np.where(peak, np.fmin(t, (gmax * F32(0.05))[:, None]), t)  # f32::min ignores NaN
    if mut == "thr_ulp_up":
        t = np.nextafter(t, F32(np.inf))
    elif mut == "thr_ulp_down":
        t = np.nextafter(t, F32(-np.inf))
    return t.astype(F32)


def row_scale(c: np.ndarray) -> np.ndarray:
    return np.fmax(np.fmax.reduce(np.abs(c), axis=1, initial=F32(0.0)), F32(1e-10)).astype(F32)  # NaN-ignoring


def keep_and_q(c: np.ndarray, thr: np.ndarray, scale: np.ndarray, mut=None) -> np.ndarray:
    """src/codec.rs:277-303 elementwise: c, thr [R, n], scale [R] -> i16 q (0 = dropped)."""
    nfl = (NOISE_FLOOR * scale)[:, None]
    a = np.abs(c)
    t = thr * scale[:, None]
    above_floor = a >= nfl if mut == "ge_noise_floor" else a > nfl
    above_thr = a >= t if mut == "ge_threshold" else a > t
    x = ((c / scale[:, None]) * F32(32768.0)).astype(np.float64)
    r = np.rint(x) if mut == "ties_even" else np.trunc(x + np.copysign(0.5, x))  # f32::round: half away from 0
    r = np.clip(r, -32768.0, 32767.0)
    return np.where(above_floor & above_thr, np.nan_to_num(r, nan=0.0), 0.0).astype(np.int16)


def quantise(c: np.ndarray, sr: int, mut=None):
    """-> (scale [R] f32, q [R, 1024] i16) for rows c [R, 1024]."""
    c = np.ascontiguousarray(c, F32)
    w, edges = perceptual(sr)
    with np.errstate(all="ignore"):
        scale = row_scale(c)
        thr = np.zeros_like(c)
        for b in range(len(edges) - 1):
            s, e = int(edges[b]), min(int(edges[b + 1]), HOP)
            if s < e:
                thr[:, s:e] = band_thresholds(c[:, s:e], w[s:e], scale, mut)
        return scale, keep_and_q(c, thr, scale, mut)


def raw_threshold(ch: int) -> F32:
    return F32(F32(FRAME * ch * 2) * F32(0.85))


def decide(nnz: np.ndarray, ch: int, mut=None) -> np.ndarray:
    """src/codec.rs:505-521: per-frame raw decision from the rows' nnz [F * ch]."""
    per = nnz.reshape(-1, ch).astype(np.int64)
    compressed = (8 + 4 * per).sum(axis=1) + 8 + 4 * ch + 64
    cf = compressed.astype(F32)
    thr = raw_threshold(ch)
    return (cf > thr) if mut == "gt_raw" else (cf >= thr)


def flip_point(ch: int) -> int:
    """Smallest total nnz of a frame that makes it raw."""
    return next(n for n in range(HOP * ch + 1) if decide(np.array([n] + [0] * (ch - 1)), ch)[0])


def sat_i16(x: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        y = np.clip(x, -32768.0, 32767.0)
    return np.where(np.isnan(y), 0.0, y).astype(np.int16)  # `as i16`: truncation, NaN -> 0


def raw_planes(stream: np.ndarray | None, n_samples: int, ch: int, frames, t0: int = 0, t_count: int | None = None):
    """src/codec.rs:496-502 (channel-planar, quirk Q1) for absolute frames, from the shard [t0, t0 + t_count)."""
    _, win, _ = O.tables()
    L = -(-n_samples // ch)
    t_count = L - t0 if t_count is None else t_count
    out = np.zeros((len(frames), ch, FRAME), np.int16)
    i = np.arange(FRAME, dtype=np.int64)
    for n, f in enumerate(frames):
        t = f * HOP + i - HOP // 2
        for c in range(ch):
            ok = (t >= 0) & (t * ch + c < n_samples) & (t >= t0) & (t - t0 < t_count)
            x = np.zeros(FRAME, F32)
            if stream is not None:
                x[ok] = stream[t[ok] * ch + c]
            with np.errstate(all="ignore"):
                out[n, c] = sat_i16((x * win) * F32(32767.0))
    return out


def build_records(ch: int, scale: np.ndarray, q: np.ndarray, is_raw: np.ndarray, planes: np.ndarray | None):
    """The fixed-size records of include/glc.h; bytes no kernel writes keep the sentinel."""
    nf, hdr = is_raw.size, header_bytes(ch)
    out = np.full((nf, record_bytes(ch)), SENTINEL, np.uint8)
    out[:, 0:4] = is_raw.astype(np.uint32)[:, None].view(np.uint8)
    out[:, 4:8] = 0
    nnz = (q != 0).sum(axis=1).astype(np.uint32)
    meta = np.empty((nf, ch, 2), np.uint32)
    meta[:, :, 0] = scale.astype(F32).view(np.uint32).reshape(nf, ch)
    meta[:, :, 1] = nnz.reshape(nf, ch)
    out[:, 8:8 + 8 * ch] = meta.reshape(nf, -1).view(np.uint8)
    pay = out[:, hdr:].view(np.int16).reshape(nf, ch, FRAME)
    comp = ~is_raw.astype(bool)
    pay[comp, :, :HOP] = q.reshape(nf, ch, HOP)[comp]
    if is_raw.any():
        pay[is_raw.astype(bool)] = planes[is_raw.astype(bool)]
    return out


# ----------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------

@dataclass
class Case:
    """Frames of coefficient rows (row m = frame * ch + c) of a stream of n_samples interleaved samples.
    The device launch covers frames [frame_begin, n_frames) from the shard [t0, L) of `stream`
    (None: silence); `expected` holds the records of ALL n_frames frames."""
    family: str
    sr: int
    ch: int
    coeffs: np.ndarray
    stream: np.ndarray | None = None
    frame_begin: int = 0
    t0: int = 0
    info: dict = field(default_factory=dict)
    expected: np.ndarray | None = None
    scale: np.ndarray | None = None
    q: np.ndarray | None = None
    is_raw: np.ndarray | None = None
    planes: np.ndarray | None = None  # raw plane of every frame [n_frames, ch, 2048]

    @property
    def n_frames(self) -> int:
        return self.coeffs.shape[0] // self.ch

    @property
    def n_samples(self) -> int:
        return self.n_frames * HOP * self.ch  # O.num_frames gives back n_frames

    @property
    def name(self) -> str:
        return f"{self.family}-{self.sr}-ch{self.ch}"


def oracle_rows(c: np.ndarray, sr: int):
    """scale, thresholds and q of every row from the C oracle (src/codec.rs:198, :188-240, :270-311)."""
    w, edges = perceptual(sr)
    R = c.shape[0]
    scale = np.empty(R, F32)
    q = np.zeros((R, HOP), np.int16)
    thr = np.empty((R, HOP), F32)
    for m in range(R):
        thr[m] = O.thresholds(c[m], w, edges)
        scale[m] = row_scale(c[m:m + 1])[0]
        idx, qq = O.compress(c[m], scale[m], thr[m])
        q[m, idx] = qq
    return scale, thr, q


def finish(case: Case) -> Case:
    """Expected records of every frame of the case: oracle rows, numpy decision and raw planes."""
    assert case.coeffs.dtype == F32 and case.coeffs.shape[0] % case.ch == 0
    assert O.num_frames(case.n_samples, case.ch) == case.n_frames
    scale, _, q = oracle_rows(case.coeffs, case.sr)
    is_raw = decide((q != 0).sum(axis=1), case.ch)
    if case.stream is None:
        planes = np.zeros((case.n_frames, case.ch, FRAME), np.int16)
    else:
        planes = raw_planes(case.stream, case.n_samples, case.ch, range(case.n_frames))
    case.scale, case.q, case.is_raw, case.planes = scale, q, is_raw, planes
    case.expected = build_records(case.ch, scale, q, is_raw, planes)
    return case


def _pad_rows(rows: np.ndarray, ch: int) -> np.ndarray:
    extra = (-rows.shape[0]) % ch
    return np.concatenate([rows, np.zeros((extra, HOP), F32)]) if extra else rows


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def _from_bits(b):
    return np.asarray(b, np.uint32).view(F32)


# --- thresholds: one bisected bin per band and row ---------------------------------------------------

_THR_ROWS = 64
# row r takes scale _THR_SCALES[(r + r // 16) % 4] (x a random factor in odd rows): every row position of a
# workgroup meets every scale.  Short low bands can hold a flip only at small scales (the bin itself sets
# their energy), the threshold decides over the noise floor only at large ones.
_THR_SCALES = (16.0, 64.0, 256.0, 1024.0)


def _keep_bin(vals, j, v, wts, scale):
    """keep decision of bin j (per row) of one band when it holds v: the ordered sum of that band only."""
    R = vals.shape[0]
    cand = vals.copy()
    cand[np.arange(R), j] = v
    with np.errstate(all="ignore"):
        t = band_thresholds(cand, wts, scale)[np.arange(R), j]
        q = keep_and_q(v[:, None], t[:, None], scale)
    return q[:, 0] != 0


def threshold_rows(sr: int, seed: int):
    """-> rows [R, 1024], flips: list of (row, bin, side, regime); side 1 = kept float, 0 = dropped float."""
    rng = np.random.default_rng(seed)
    w, edges = perceptual(sr)
    nb = len(edges) - 1
    R = _THR_ROWS
    scale = np.array([_THR_SCALES[(r + r // 16) % 4] * (1.0 if r % 2 == 0 else 1.0 + 0.37 * rng.random())
                      for r in range(R)], F32)
    rows = np.zeros((R, HOP), F32)
    # fillers: random values below the noise floor (dropped, but part of every band sum, in random order of size)
    v = np.exp(rng.uniform(np.log(1e-4), np.log(3.9e-3), (R, nb)))
    for b in range(nb):
        s, e = int(edges[b]), int(edges[b + 1])
        rows[:, s:e] = (rng.uniform(-1.0, 1.0, (R, e - s)) * (v[:, b] * scale)[:, None]).astype(F32)
    # the row maximum (its scale) sits in the longest band, where it adds least to the band's energy
    max_band = np.full(R, int(np.argmax(np.diff(edges.astype(np.int64)))))
    max_bin = np.array([rng.integers(edges[b], edges[b + 1]) for b in max_band])
    rows[np.arange(R), max_bin] = scale * np.where(rng.random(R) < 0.5, F32(-1.0), F32(1.0))
    flips = []
    for b in range(nb):
        s, e = int(edges[b]), int(edges[b + 1])
        j = rng.integers(0, e - s, R)
        clash = (max_band == b) & (j == max_bin - s)
        j[clash] = (j[clash] + 1) % (e - s)
        ok = ~((max_band == b) & (e - s == 1))
        band = rows[:, s:e]
        lo = np.zeros(R, np.uint32)
        hi = _bits(scale * F32(0.29)).copy()
        ok &= _keep_bin(band, j, _from_bits(hi), w[s:e], scale) & ~_keep_bin(band, j, _from_bits(lo), w[s:e], scale)
        for _ in range(32):
            mid = ((lo.astype(np.uint64) + hi) // 2).astype(np.uint32)
            k = _keep_bin(band, j, _from_bits(mid), w[s:e], scale)
            lo, hi = np.where(k, lo, mid), np.where(k, mid, hi)
        ok &= (hi - lo == 1)
        side = (np.arange(R) // 16 + b) % 2  # independent of the scale: both sides at every scale
        sign = np.where(rng.random(R) < 0.5, F32(-1.0), F32(1.0))
        val = _from_bits(np.where(side == 1, hi, lo)) * sign
        # threshold decides when the edge lies above the noise floor
        regime = np.where(_from_bits(lo) > NOISE_FLOOR * scale, "thr", "floor")
        for r in np.nonzero(ok)[0]:
            rows[r, s + j[r]] = val[r]
            flips.append((int(r), s + int(j[r]), int(side[r]), str(regime[r])))
    return rows, flips


# --- noise floor, peak gate, rounding, extremes ------------------------------------------------------

def noise_floor_rows(sr: int, seed: int):
    """Rows with one bin at exactly f32(noise_floor * scale) and one at the next float up, in a quiet band."""
    rng = np.random.default_rng(seed)
    w, edges = perceptual(sr)
    nb = len(edges) - 1
    rows, marks = [], []
    for r, s in enumerate((1.0, 3.0, 64.0, 0.37, 1.0e-3, 17.25, 2.0, 0.5)):
        for sign in (1.0, -1.0):
            c = np.zeros(HOP, F32)
            b = (3 * r + (sign < 0)) % nb
            if edges[b + 1] - edges[b] < 2:
                b = nb - 1
            lo, hi = int(edges[b]), int(edges[b + 1])
            pin_band = (b + nb // 2) % nb if nb > 1 else b
            pin = int(edges[pin_band]) if pin_band != b else hi - 1
            c[pin] = F32(s) * F32(sign)
            x, y = rng.choice([k for k in range(lo, hi) if k != pin], 2, replace=False)
            nfl = F32(NOISE_FLOOR * F32(s))
            c[x] = nfl * F32(sign)
            c[y] = np.nextafter(nfl, F32(np.inf)) * F32(sign)
            rows.append(c)
            marks.append((len(rows) - 1, int(x), int(y)))
    return np.array(rows), marks


def peak_gate_rows(seed: int):
    """192 kHz: the last band nearly full at ~scale, one bin near its top at f32(scale * 0.3) (not a peak, the
    band's threshold drops it) or at the next float up (a peak, the capped threshold keeps it).  Each row
    is followed by a partner row, so a 2- or 3-channel frame stays compressed."""
    sr = 192000
    rng = np.random.default_rng(seed)
    w, edges = perceptual(sr)
    s0, e0 = int(edges[-2]), int(edges[-1])
    cand, where = [], []
    for s in (4.0, 4.5, 5.0, 5.5):
        for f in np.linspace(0.85, 1.0, 16):
            for top in range(1, 9):
                S, k = F32(s), e0 - top
                c = np.zeros(HOP, F32)
                c[s0:e0] = F32(f) * S
                c[0] = S
                g = F32(S * F32(0.3))
                a, b = c.copy(), c.copy()
                a[k], b[k] = g, np.nextafter(g, F32(np.inf))
                cand += [a, b]
                where.append(k)
    _, q = quantise(np.array(cand), sr)
    found = [(cand[2 * i], cand[2 * i + 1], k) for i, k in enumerate(where) if q[2 * i, k] == 0 and q[2 * i + 1, k] != 0]
    assert found, "no (scale, fill, bin) puts the peak gate on the keep / drop edge"
    pick = [found[i] for i in rng.choice(len(found), min(6, len(found)), replace=False)]
    rows, marks = [], []
    partner = np.zeros(HOP, F32)
    partner[5] = F32(0.75)
    for a, b, k in pick:
        for x in (a, b):
            rows += [x, partner]
            marks.append((len(rows) - 2, k))
    return np.array(rows), marks


def rounding_rows(seed: int):
    """scale 1.0: c = +-(k + 0.5) / 32768 and both floats beside it, +-1.0, the float below 1.0."""
    rng = np.random.default_rng(seed)
    ks = np.concatenate([[131, 132, 1000, 1001, 16383, 16384, 32765, 32766, 32767],
                         rng.integers(131, 32767, 60)])
    bins = np.arange(12, 230, 4)  # weight 1.0 at 44.1 kHz, sparse: the threshold stays under the noise floor
    rows, expect = [], []          # expect: (row, bin, q)
    vals = []
    for k in ks:
        for sign in (1.0, -1.0):
            c = F32(sign * (k + 0.5) / 32768.0)
            vals.append((c, sign * (k + 1)))
            vals.append((np.nextafter(c, F32(0.0)), sign * k))
            vals.append((np.nextafter(c, F32(sign * np.inf)), sign * (k + 1)))
    vals.append((np.nextafter(F32(1.0), F32(0.0)), 32767))
    vals.append((np.nextafter(F32(-1.0), F32(0.0)), -32768))
    per = len(bins)
    for i in range(0, len(vals), per):
        c = np.zeros(HOP, F32)
        c[2] = F32(1.0) if (i // per) % 2 == 0 else F32(-1.0)  # the row maximum: scale 1.0
        expect.append((len(rows), 2, 32767 if c[2] > 0 else -32768))
        for n, (v, qv) in enumerate(vals[i:i + per]):
            c[bins[n]] = v
            expect.append((len(rows), int(bins[n]), int(min(max(qv, -32768), 32767))))
        rows.append(c)
    return np.array(rows), expect


def extreme_rows(sr: int, seed: int):
    """-> rows, names: zero, subnormal, repeated negative maximum, overflowing band energy, NaN, inf."""
    rng = np.random.default_rng(seed)
    _, edges = perceptual(sr)
    rows, names = [], []

    def add(c, name):
        rows.append(c.astype(F32))
        names.append(name)

    add(np.zeros(HOP, F32), "zero")
    sub = _from_bits(rng.integers(1, 0x800000, HOP).astype(np.uint32)) * np.where(rng.random(HOP) < 0.5, -1, 1).astype(F32)
    add(sub, "subnormal")
    c = (rng.uniform(-0.5, 0.5, HOP)).astype(F32)
    c[rng.choice(HOP, 5, replace=False)] = F32(-0.875)
    add(c, "negative_max")
    for s in (3.0e19, 8.0e18):  # squares overflow to inf one by one / only their sum does
        c = (rng.uniform(-1.0, 1.0, HOP) * s * 1e-3).astype(F32)
        c[300:420] = (rng.uniform(0.4, 1.0, 120) * s).astype(F32)
        c[350] = F32(s)
        add(c, "overflow")
    def band_around(k):  # a band of two bins or more, at bin k or after it
        b = int(np.searchsorted(edges, k, side="right")) - 1
        while edges[b + 1] - edges[b] < 2:
            b += 1
        return int(edges[b]), int(edges[b + 1])

    lo, hi = band_around(110)
    c = (rng.uniform(-0.02, 0.02, HOP)).astype(F32)
    c[lo:hi] = rng.uniform(-0.2, 0.2, hi - lo).astype(F32)
    c[lo], c[hi - 1] = F32(np.nan), F32(1.0)  # a NaN and a peak in one band
    add(c, "nan")
    lo, hi = band_around(0)
    c = (rng.uniform(-0.1, 0.1, HOP)).astype(F32)
    c[hi - 1], c[lo], c[500] = F32(np.nan), F32(-0.6), F32(0.31)
    add(c, "nan_low_band")
    c = (rng.uniform(-1.0, 1.0, HOP)).astype(F32)
    c[640] = F32(np.inf)
    add(c, "inf")
    return np.array(rows), names


# --- raw decision ------------------------------------------------------------------------------------

def _split(total: int, ch: int, rng) -> list:
    """An uneven split of `total` kept bins over `ch` rows of at most 1024 (some empty, some full)."""
    counts, rem = [0] * ch, total
    for n, c in enumerate(rng.permutation(ch)):
        lo, hi = max(0, rem - HOP * (ch - n - 1)), min(HOP, rem)
        counts[c] = int((lo, hi, rng.integers(lo, hi + 1))[rng.integers(0, 3)])
        rem -= counts[c]
    assert rem == 0
    return counts


def _row_with_nnz(n: int, rng) -> np.ndarray:
    """A row that keeps exactly n coefficients: all of them peaks of a scale-1.0 row."""
    c = np.zeros(HOP, F32)
    if n:
        idx = rng.choice(HOP, n, replace=False)
        c[idx] = (rng.uniform(0.31, 1.0, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(F32)
        c[idx[0]] = F32(1.0)
    return c


RAW_LEAD = 2                       # frames before the launch's first frame
RAW_PATTERN = (-1, 0, -1, 1, 0, -1, 1, -1, 0, 1, -1, 0, 0, -1, 1, 1)  # total nnz = flip point + this, frame by frame


def raw_case(ch: int, sr: int, seed: int) -> Case:
    rng = np.random.default_rng(seed)
    flip = flip_point(ch)
    totals = [max(0, flip - 300)] * RAW_LEAD + [flip + d for d in RAW_PATTERN]
    rows = np.concatenate([[_row_with_nnz(n, rng) for n in _split(t, ch, rng)] for t in totals]).astype(F32)
    nf = len(totals)
    L = nf * HOP
    x = (rng.standard_normal(L * ch) * 0.7).astype(F32)
    special = rng.choice(L * ch, L * ch // 12, replace=False)
    x[special] = rng.choice(np.array([1.5, -1.5, 3.0, -7.0, np.inf, -np.inf, np.nan], F32), special.size)
    t0 = RAW_LEAD * HOP - HOP // 2
    case = Case("raw", sr, ch, rows, stream=x, frame_begin=RAW_LEAD, t0=t0,
                info=dict(flip=flip, totals=totals))
    return finish(case)


# --- the case list -------------------------------------------------------------------------------------

def _case(family, sr, ch, rows, **info) -> Case:
    return finish(Case(family, sr, ch, _pad_rows(np.ascontiguousarray(rows, F32), ch), info=info))


def threshold_case(sr: int, ch: int = 1) -> Case:
    rows, flips = threshold_rows(sr, seed=1000 + sr)
    return _case("thresholds", sr, ch, rows, flips=flips)


def build_cases() -> list:
    cases = [threshold_case(sr) for sr in RATES]
    for sr in (44100, 192000):
        for ch in (2, 3, 5):
            cases.append(threshold_case(sr, ch))
    for sr in (44100, ODD_RATE):
        rows, marks = noise_floor_rows(sr, seed=7 + sr)
        for ch in (1, 3):
            cases.append(_case("noise_floor", sr, ch, rows, marks=marks))
    rows, marks = peak_gate_rows(seed=11)
    for ch in (2, 3):
        c = _case("peak_gate", 192000, ch, rows, marks=marks)
        cases.append(c)
    rows, expect = rounding_rows(seed=13)
    for ch in (1, 4, 6):
        cases.append(_case("rounding", 44100, ch, rows, expect=expect))
    for sr in (44100, ODD_RATE):
        rows, names = extreme_rows(sr, seed=17 + sr)
        for ch in (1, 2, 7):
            cases.append(_case("extremes", sr, ch, rows, names=names))
    for ch in CHANNELS:
        cases.append(raw_case(ch, 44100, seed=100 + ch))
    cases.append(raw_case(2, 192000, seed=300))
    cases.append(raw_case(5, ODD_RATE, seed=301))
    return cases


_cached = None


def cases() -> list:
    global _cached
    if _cached is None:
        _cached = build_cases()
    return _cached


def digest(cs) -> str:
    h = hashlib.sha256()
    for c in cs:
        h.update(c.name.encode())
        h.update(c.coeffs.tobytes())
        if c.stream is not None:
            h.update(c.stream.tobytes())
    return h.hexdigest()
