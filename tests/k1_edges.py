"""Deterministic PCM that sits on the value and layout edges of the forward transform (K1), which kernel each
launch is meant for, and the coefficient bits every launch must give (test helper: numpy + the CPU oracle only).

K1 (csrc/glc_mdct_fwd.hpp) is six kernels behind one dispatch by row count (launch_mdct_forward) - the 2 x 2 and
2 x 4 short-clip kernels, the 64 x 128 round kernel, the 256-row kernels with 8 and 16 waves and the 128 x 128
kernel before them - each with its own multiply / add step and each with two PCM loaders (one dwordx4 per frame
segment for 1 / 2 / 4 / 8 channels, one dword per (row, sample) otherwise).  Audio reaches few of their edges.
The families built here reach them on purpose:

  values    one stream per channel count with a STATION every few frames: a window holding unit impulses at the
            first and last step of a 16- and 32-step stage and at the hop boundary, subnormals, products that
            are subnormal, -0.0, zeros, +-3e38, +-inf, quiet / signalling NaNs - in row 0 and in the last row of
            32- and 256-row tiles - through every kernel and both loaders
  all_rows  tonal-plus-noise streams at every row count at which the dispatch changes kernel, every row compared
  channels  the per-row loader at >= 4096 rows with 5 .. 300 channels (tiles that start mid-frame; a tile inside
            one frame), ragged last sample frame
  guards    tight shards in the middle of a stream, with 0 / 1 / 3 / 5 samples of extra halo, NaN around the shard
            and a sentinel around the coefficient destination
  far       shards late in VIRTUAL streams of more than 2^32 samples: only the shard exists, t0 is huge

Expected coefficients are the C oracle's (`encode_range_records(..., taps=True)`), over all rows of a launch
(`expected`) or over a few rows (`oracle_rows`).  `model` restates the transform in numpy float32 on a few rows
of a case, with optional single-edit mutations (MUTATIONS) - each the kind of edit an optimisation makes; each
must change some expected word, which is what shows that the families would notice it in a kernel.

NaN rows: a row whose window holds ONE NaN bit pattern (a signalling one is quieted by the first multiply), or
whose sum runs into inf - inf, has bits the reference defines, and is compared like any other.  A row in which
two DIFFERENT NaN patterns meet (a NaN running sum and a NaN product) has not: which payload an add returns
depends on the operand order the compiler picked, for gcc, numpy and rustc alike.  The two stations named
`unpinned-*` are such rows, on purpose; `unpinned_rows` lists them.
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle as O

F32 = np.float32
HOP, FRAME = 1024, 2048
SENTINEL_BITS = 0x7FC00ABC           # a NaN no arithmetic produces: "never written"
POISON_BITS = 0x7FC00000             # what the oracle puts where a stream has samples the shard does not hold
QNAN, SNAN, NAN_B = 0x7FC00001, 0x7F800001, 0xFFC12345
PINF, NINF, NEG_ZERO = 0x7F800000, 0xFF800000, 0x80000000
I_POS = (0, 1, 15, 16, 31, 32, 1023, 1024, 2047)   # first / last step of a 16- and 32-step stage, the hop boundary
SEG_CHANNELS = (1, 2, 4, 8)          # channel counts with a segment loader
HALOS = (0, 1, 3, 5)                 # guards: samples in front of the tight shard
STATION_LIMIT = 600                  # stations sit in the first rows of a launch: below every values row count

# include/glc_debug.h glc_debug_set_mdct_variant
VARIANT = {"dma": 1, "st8": 2, "st16": 3, "sched": 4}
LARGE = (("dma", 1), ("st8", 2), ("st16", 3))

# the row counts at which launch_mdct_forward changes kernel: smallest / largest M of each (segment loader | other)
TABLE = {
    "small2": ((1, 31, 33, 640), (639,)),
    "small4": ((641, 3583), (4095,)),
    "sched": ((1793, 2048, 2047), (1794,)),
    "large": ((3584, 3584 + 255, 4097), (4096, 4096 + 257)),
}

MUTATIONS = ("fma", "two_accumulators", "descending_i", "neg_zero_init", "subnormal_inputs_zero",
             "subnormal_products_zero", "norm_in_table", "window_in_table", "stages_swapped", "padding_reads_neighbour",
             "ragged_frame_dropped", "channel_off_by_one_above_256")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def word(x) -> int:
    """The bit pattern of one float."""
    return int(F32(x).view(np.uint32))


def kernel_for(M: int, ch: int, variant: int) -> str:
    """launch_mdct_forward (csrc/glc_kernels.hip), restated."""
    seg = ch in SEG_CHANNELS
    if M <= 640:
        return "small2"
    if variant == 4 and 1792 < M <= 2048:
        return "sched"
    if M < (3584 if seg else 4096):
        return "small4"
    if variant in (1, 2, 3):
        return ("dma", "st8", "st16")[variant - 1]
    last_round = ((M + 255) // 256) % 32
    return "st16" if last_round == 0 or last_round > 16 else "st8"


def num_frames(n_samples: int, ch: int) -> int:
    return -(-(512 + -(-n_samples // ch)) // 1024) - 1


# ----------------------------------------------------------------------------------------------------
# sources and cases
# ----------------------------------------------------------------------------------------------------

class Source:
    """Per-channel samples [t0, t0 + count) of a stream of n_samples interleaved floats - all that exists of it."""

    def __init__(self, key, sr, ch, n_samples, t0, data):
        self.key, self.sr, self.ch, self.n_samples, self.t0 = key, sr, ch, n_samples, t0
        self.data = np.ascontiguousarray(data, F32).reshape(-1)
        self.per_channel = -(-n_samples // ch)
        self.n_frames = num_frames(n_samples, ch)
        assert self.data.size <= n_samples - t0 * ch

    def window(self, f0, f1, halo=0):
        """(t0, t_count) of the tight shard of frames [f0, f1), `halo` samples more in front."""
        lo = max(0, f0 * HOP - 512 - halo)
        hi = min(self.per_channel, (f1 - 1) * HOP - 512 + FRAME)
        return lo, hi - lo

    def shard(self, t0, t_count):
        lo = (t0 - self.t0) * self.ch
        hi = min((t0 + t_count) * self.ch, self.n_samples) - self.t0 * self.ch
        assert 0 <= lo <= hi <= self.data.size, "the source does not hold this shard"
        return self.data[lo:hi]


@dataclass
class Case:
    """Frames [f0, f1) of `src` from its tight shard; `targets` = ((kernel, variant), ...): the kernels the launch is
    meant for and the debug variant that reaches each (0: the dispatch by row count); `span`: the frame range whose
    oracle output this case shares with its neighbours (None: its own)."""
    name: str
    family: str
    src: Source
    f0: int
    f1: int
    targets: tuple
    span: tuple = None
    info: dict = field(default_factory=dict)

    @property
    def ch(self):
        return self.src.ch

    @property
    def M(self):
        return (self.f1 - self.f0) * self.src.ch

    def shard(self, halo=0):
        """(pcm, t0, t_count)"""
        t0, tc = self.src.window(self.f0, self.f1, halo)
        return self.src.shard(t0, tc), t0, tc


def _content(sr, ch, t_lo, count, seed):
    """Tonal plus noise, as test_gpu_parity._k1_stream: a sine per channel, noise bursts in the middle and near the
    end (raw frames), activity at the end; phases so that no sample is an exact zero."""
    rng = np.random.default_rng(seed)
    t = (t_lo + np.arange(count, dtype=np.float64))[:, None]
    x = (np.sin(2 * np.pi * rng.uniform(60, 9000, (1, ch)) * t / sr + rng.uniform(0.1, 3.0, (1, ch))) * 0.4).astype(F32)
    mid, nb = count // 2, min(6000, count // 4)
    x[mid:mid + nb] = rng.standard_normal((nb, ch)).astype(F32) * F32(0.3)
    ne = min(3000, count // 4)
    x[-ne - nb:-ne] = rng.standard_normal((nb, ch)).astype(F32) * F32(0.3)      # and one that the last frames hold
    x[-ne:] += rng.standard_normal((ne, ch)).astype(F32) * F32(0.2)
    return x


def _whole_stream(key, ch, frames, seed, sr=48000):
    """A stream of `frames` frames from sample 0, ragged: the last sample frame holds channel 0 only."""
    n = frames * HOP * ch - 300 * ch - (ch - 1)
    src = Source(key, sr, ch, n, 0, _content(sr, ch, 0, frames * HOP, seed).reshape(-1)[:n])
    assert src.n_frames == frames and n % ch == (1 if ch > 1 else 0)
    return src


def _targets(M, ch, kernels):
    t = tuple((k, VARIANT.get(k, 0)) for k in kernels)
    for k, v in t:
        assert kernel_for(M, ch, v) == k, (M, ch, k)
    return t


def _class_targets(cls, M, ch):
    if cls == "large":
        return _targets(M, ch, ("dma", "st8", "st16"))
    if cls == "sched":
        return _targets(M, ch, ("sched", "small4"))     # the same rows through the kernel the dispatch picks alone
    return _targets(M, ch, (cls,))


def _near(M, ch, at_least):
    """The multiple of ch nearest to M that is not below `at_least`."""
    lo, hi = M // ch * ch, -(-M // ch) * ch
    c = [m for m in (lo, hi) if m >= at_least]
    return min(c, key=lambda m: abs(m - M))


# ----------------------------------------------------------------------------------------------------
# values: stations
# ----------------------------------------------------------------------------------------------------

STATIONS = tuple(f"impulse-i{i}" for i in I_POS) + (
    "subnormal-window", "subnormal-mixed", "tiny-at-ends", "negative-zero", "zero", "zero-signed-against-column-0", "huge",
    "plus-inf", "minus-inf", "inf-minus-inf", "quiet-nan", "signalling-nan", "nan-then-inf-minus-inf",
    "unpinned-two-nan-payloads", "unpinned-inf-minus-inf-then-nan")
ZERO_STATIONS = ("negative-zero", "zero", "zero-signed-against-column-0")     # every coefficient +0.0
# window positions of the samples that make a station's row undefined: a row that sees ALL of them is unpinned
UNPINNED = {"unpinned-two-nan-payloads": (100, 200), "unpinned-inf-minus-inf-then-nan": (100, 150, 300)}


def _station_window(name, base, rng):
    """The 2048 samples (as bits) of one channel over the station's frame; `base` is the stream's own content."""
    u = bits(base).copy()
    if name.startswith("impulse-i"):
        i = int(name[9:])
        u[:] = 0
        u[i] = word(1.0 if I_POS.index(i) % 2 == 0 else -1.0)
    elif name == "subnormal-window":
        u[:] = rng.integers(1, 1 << 23, FRAME).astype(np.uint32) | (rng.integers(0, 2, FRAME).astype(np.uint32) << 31)
    elif name == "subnormal-mixed":  # beside normals small enough (2e-38 .. 1.2e-37) for a subnormal term to show in the sum
        u[::2] = rng.integers(1, 1 << 23, HOP).astype(np.uint32) | (rng.integers(0, 2, HOP).astype(np.uint32) << 31)
        u[1::2] = bits(np.copysign(F32(2e-38) + np.abs(base[1::2]) * F32(2.5e-37), base[1::2]))
    elif name == "tiny-at-ends":     # 1e-36 * w[0] = 7.7e-40: the windowed sample itself is subnormal
        u[:] = 0
        u[:8] = u[-8:] = word(1e-36)
        u[4] = u[-4] = word(-1e-36)
    elif name == "negative-zero":
        u[:] = NEG_ZERO
    elif name == "zero":
        u[:] = 0
    elif name == "zero-signed-against-column-0":   # every product of coefficient 0 is -0.0: the sum must still start at +0.0
        T, _, _ = O.tables()
        u[:] = np.where(T[0] > 0, NEG_ZERO, 0).astype(np.uint32)
    elif name == "huge":             # the running sum overflows mid-way, then meets the other sign
        u[:] = 0
        u[500:504] = word(3e38)
        u[900:904] = word(-3e38)
        u[1500] = word(3e38)
    elif name == "plus-inf":
        u[700] = PINF
    elif name == "minus-inf":
        u[700] = NINF
    elif name == "inf-minus-inf":
        u[300], u[1300] = PINF, NINF
    elif name == "quiet-nan":
        u[100] = QNAN
    elif name == "signalling-nan":
        u[100] = SNAN
    elif name == "nan-then-inf-minus-inf":
        u[100], u[300], u[400] = QNAN, PINF, NINF
    elif name == "unpinned-two-nan-payloads":
        u[100], u[200] = QNAN, NAN_B
    elif name == "unpinned-inf-minus-inf-then-nan":
        u[100], u[150], u[300] = PINF, NINF, QNAN
    else:
        raise KeyError(name)
    return u


def _station_rows(ch):
    """Launch-relative row of each station: row 0 and the last row of a 32-row and of a 256-row tile first, then
    the other first / last rows of 32-row tiles; stations of one channel at least three frames apart, so that no
    row sees two of them."""
    anchors = [0, 31, 255, 256, 32] + [r for r in range(STATION_LIMIT) if r % 32 in (0, 31) and r not in (0, 31, 32, 255, 256)]
    taken, out = [], {}
    it = iter(anchors)
    for name in STATIONS:
        for r in it:
            f, c = divmod(r, ch)
            if all(c != c2 or abs(f - f2) >= 3 for f2, c2 in taken):
                taken.append((f, c))
                out[name] = r
                break
        else:
            raise AssertionError("not enough anchor rows")
    return out


VALUES_F0 = 3        # every values launch starts at this frame (a shard that begins mid-stream)


def _values_source(ch, frames):
    src = _whole_stream(f"values-ch{ch}", ch, frames, 300 + ch)
    rng = np.random.default_rng(350 + ch)
    u = src.data.view(np.uint32)
    rows = _station_rows(ch)
    for name in STATIONS:
        f, c = divmod(rows[name], ch)
        a = (VALUES_F0 + f) * HOP - 512
        sl = slice(a * ch + c, (a + FRAME) * ch + c, ch)
        u[sl] = _station_window(name, u[sl].view(F32), rng)
    return src, rows


def _values_family():
    cases = []
    shapes = {2: (("small2", 640), ("small4", 642), ("sched", 2048), ("large", 3584)),
              3: (("small2", 639), ("small4", 4095), ("sched", 1794), ("large", 4098)),
              8: (("large", 3584),)}
    for ch, todo in shapes.items():
        frames = max(M for _, M in todo) // ch
        src, rows = _values_source(ch, VALUES_F0 + frames + 2)
        for cls, M in todo:
            assert M % ch == 0 and M > STATION_LIMIT
            cases.append(Case(f"values-ch{ch}-{cls}-{M}", "values", src, VALUES_F0, VALUES_F0 + M // ch,
                              _class_targets(cls, M, ch), span=(VALUES_F0, VALUES_F0 + frames), info=dict(stations=rows, cls=cls)))
    return cases


def station_rows(case) -> dict:
    return case.info.get("stations", {})


def unpinned_rows(case) -> list:
    """Rows of a values case in which two different NaN patterns meet: the station's own row and, its marked
    samples lying in the first half of the window, the row of the frame before."""
    out = []
    for name, pos in UNPINNED.items():
        r = station_rows(case).get(name)
        if r is None:
            continue
        assert max(pos) < HOP
        out += [x for x in (r - case.ch, r) if 0 <= x < case.M]
    return sorted(out)


# ----------------------------------------------------------------------------------------------------
# the other families
# ----------------------------------------------------------------------------------------------------

def _all_rows_family():
    cases = []
    src1 = _whole_stream("all-ch1", 1, 4097, 401)
    for cls, (seg, _) in TABLE.items():
        for M in seg:
            cases.append(Case(f"all-ch1-{cls}-{M}", "all_rows", src1, 0, M, _class_targets(cls, M, 1), span=(0, 4097), info=dict(cls=cls)))
    src3 = _whole_stream("all-ch3", 3, 1451, 403)
    for cls, (_, other) in TABLE.items():
        for M in other:
            M3 = _near(M, 3, 4096 if cls == "large" else 0)
            cases.append(Case(f"all-ch3-{cls}-{M3}", "all_rows", src3, 0, M3 // 3, _class_targets(cls, M3, 3), span=(0, 1451), info=dict(cls=cls)))
    for ch, M in ((2, 3584), (4, 3584 + 256), (8, 4104)):      # the other segment-loader shapes of the large kernels
        src = _whole_stream(f"all-ch{ch}", ch, M // ch, 400 + ch)
        cases.append(Case(f"all-ch{ch}-large-{M}", "all_rows", src, 0, M // ch, _class_targets("large", M, ch), info=dict(cls="large")))
    return cases


CHANNEL_COUNTS = (5, 6, 7, 12, 33, 257, 300)


def _channels_family():
    cases = []
    for ch in CHANNEL_COUNTS:
        frames = -(-4096 // ch)
        src = _whole_stream(f"channels-ch{ch}", ch, frames, 500 + ch)
        cases.append(Case(f"channels-ch{ch}-large-{frames * ch}", "channels", src, 0, frames, _class_targets("large", frames * ch, ch), info=dict(cls="large")))
    for ch in (5, 33):
        frames = -(-641 // ch)
        src = _whole_stream(f"channels-ch{ch}-short", ch, frames, 550 + ch)
        cases.append(Case(f"channels-ch{ch}-small4-{frames * ch}", "channels", src, 0, frames, _class_targets("small4", frames * ch, ch), info=dict(cls="small4")))
    return cases


def _guards_family():
    cases = []
    f0 = 7
    # (sched: 28 of its 64-row tiles and two rows, the fewest rows the dispatch gives it that end inside a tile)
    for ch, todo in ((2, (("small2", 66), ("sched", 1794), ("large", 4098))), (3, (("small4", 645), ("large", 4101)))):
        frames = max(M for _, M in todo) // ch
        src = _whole_stream(f"guards-ch{ch}", ch, f0 + frames + 9, 600 + ch)
        for cls, M in todo:
            assert M % ch == 0 and M % 32 and M % 256           # a partial last tile
            c = Case(f"guards-ch{ch}-{cls}-{M}", "guards", src, f0, f0 + M // ch, _class_targets(cls, M, ch),
                     span=(f0, f0 + frames), info=dict(cls=cls, halos=HALOS))
            assert c.f1 < src.n_frames
            cases.append(c)
    return cases


FAR_STREAMS = {"a": (2, (1 << 32) + 7), "b": (2, (1 << 33) + 12345), "c": (3, 3 * (1 << 33) + 5)}
FAR_ROWS = {2: (("small2", 640), ("small4", 3582), ("sched", 2048), ("large", 3584)),
            3: (("small2", 639), ("small4", 4095), ("sched", 1794), ("large", 4098))}


def _far_family():
    cases = []
    sr = 96000
    for where, key in (("mid", "a"), ("last", "b"), ("mid", "c"), ("last", "c")):
        ch, n = FAR_STREAMS[key]
        nf = num_frames(n, ch)
        kmax = max(M for _, M in FAR_ROWS[ch]) // ch
        cross = (1 << 32) // (HOP * ch * 4)                     # the last frame whose f * 1024 * ch * 4 is <= 2^32
        F0 = nf - kmax if where == "last" else cross - kmax // 2
        L = -(-n // ch)
        t_lo, t_hi = F0 * HOP - 512, min(L, (F0 + kmax - 1) * HOP - 512 + FRAME)
        data = _content(sr, ch, t_lo, t_hi - t_lo, 700 + len(cases)).reshape(-1)[:n - t_lo * ch]
        src = Source(f"far-{key}-{where}", sr, ch, n, t_lo, data)
        for cls, M in FAR_ROWS[ch]:
            k = M // ch
            f0 = nf - k if where == "last" else cross - k // 2
            cases.append(Case(f"far-{key}-{where}-{cls}-{M}", "far", src, f0, f0 + k, _class_targets(cls, M, ch),
                              span=(F0, F0 + kmax), info=dict(cls=cls, where=where, cross=cross)))
    return cases


def build_cases():
    return _values_family() + _all_rows_family() + _channels_family() + _guards_family() + _far_family()


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = build_cases()
    return _cases


def digest(cs) -> str:
    h = hashlib.sha256()
    for c in cs:
        h.update(repr((c.name, c.family, c.src.key, c.src.n_samples, c.src.t0, c.f0, c.f1, c.targets, c.span)).encode())
        h.update(hashlib.sha256(c.src.data.tobytes()).digest())
    return h.hexdigest()


# ----------------------------------------------------------------------------------------------------
# expected bits: the C oracle
# ----------------------------------------------------------------------------------------------------

_span_cache: dict = {}


def expected(case, records=False):
    """Coefficients [M, 1024] of every row of the launch (and the frame records) from encode_range_records over the
    case's span, computed from the span's tight shard; the last six spans are kept (cases that share one are
    neighbours in build_cases, and the guards and far families, which several tests walk, have six between them)."""
    F0, F1 = case.span or (case.f0, case.f1)
    key = (case.src.key, F0, F1)
    if key not in _span_cache:
        while len(_span_cache) >= 6:
            _span_cache.pop(next(iter(_span_cache)))
        src = case.src
        t0, tc = src.window(F0, F1)
        rec, taps = O.encode_range_records(src.shard(t0, tc), t0, tc, src.n_samples, src.sr, src.ch, F0, F1, taps=True)
        _span_cache[key] = (rec, taps.coeffs, taps.is_raw)
    rec, coeffs, is_raw = _span_cache[key]
    ch, rb = case.ch, O.record_bytes(case.ch)
    co = coeffs[(case.f0 - F0) * ch:(case.f1 - F0) * ch]
    if records:
        return co, rec[(case.f0 - F0) * rb:(case.f1 - F0) * rb], is_raw[case.f0 - F0:case.f1 - F0]
    return co


def oracle_rows(case, rows) -> np.ndarray:
    """The C oracle's coefficients of a few rows of a case: encode_range_records over the frames that hold them,
    in runs (frames less than 8 apart share a call), each from the case's own shard."""
    rows = np.asarray(rows)
    ch = case.ch
    frames = np.unique(rows // ch)
    runs, a = [], 0
    for j in range(1, frames.size + 1):
        if j == frames.size or frames[j] - frames[j - 1] > 8:
            runs.append((int(frames[a]), int(frames[j - 1]) + 1))
            a = j
    pcm, t0, tc = case.shard()
    out = np.empty((rows.size, HOP), F32)
    for fa, fb in runs:
        _, taps = O.encode_range_records(pcm, t0, tc, case.src.n_samples, case.src.sr, ch, case.f0 + fa, case.f0 + fb, taps=True)
        sel = (rows // ch >= fa) & (rows // ch < fb)
        out[sel] = taps.coeffs[rows[sel] - fa * ch]
    return out


def subset_rows(case, limit=64) -> np.ndarray:
    """At most `limit` rows of a case: every station row and the rows beside the unpinned ones, the first and last
    rows (leading padding, ragged end, channel 0 of the last frame), both sides of the 32- and 256-row tile edges, and
    a few at random from the first, the middle and the last frame."""
    M, ch = case.M, case.ch
    want = list(station_rows(case).values()) + unpinned_rows(case)
    want += [0, 1, ch - 1, M - 1, M - 2, M - ch, 31, 32, 255, 256, M // 2]
    rng = np.random.default_rng(M * 1000 + ch)
    for f in (0, (M // ch) // 2, M // ch - 1):           # the oracle computes whole frames: stay within three
        want += (f * ch + rng.integers(0, ch, 4)).tolist()
    out = []
    for r in want:
        if 0 <= r < M and r not in out:
            out.append(int(r))
    return np.sort(np.array(out[:limit], np.int64))


# ----------------------------------------------------------------------------------------------------
# numpy model of the transform, with single-edit mutations
# ----------------------------------------------------------------------------------------------------

def load_rows(case, rows, mut=None) -> np.ndarray:
    """The 2048 samples of each row as K1 must read them (src/codec.rs:426-481): channel c of frame f is samples
    [1024 f - 512, 1024 f + 1536) of that channel, +0.0 in front of the stream and behind the channel's last sample;
    a sample the stream has but the shard does not comes out as the oracle's poison."""
    pcm, t0, tc = case.shard()
    ch, n = case.ch, case.src.n_samples
    rows = np.asarray(rows, np.int64)
    f, c = case.f0 + rows // ch, rows % ch
    if mut == "channel_off_by_one_above_256" and ch > 256:
        c = (c + 1) % ch
    t = f[:, None] * HOP - 512 + np.arange(FRAME, dtype=np.int64)[None, :]
    length = (n - c + ch - 1) // ch                       # samples of channel c
    if mut == "ragged_frame_dropped":
        length = np.full_like(c, n // ch)
    if mut == "padding_reads_neighbour":
        t = np.clip(t, 0, length[:, None] - 1)
    real = (t >= 0) & (t < length[:, None])
    held = real & (t >= t0) & (t < t0 + tc)
    out = np.zeros(t.shape, np.uint32)
    out[real & ~held] = POISON_BITS
    e = (t - t0) * ch + c[:, None]
    out[held] = pcm.view(np.uint32)[e[held]]
    return out.view(F32)


_tt = None


def _flush(a):
    return np.where(np.abs(a) < np.finfo(F32).tiny, np.copysign(F32(0), a), a).astype(F32)


def model(case, rows, mut=None) -> np.ndarray:
    """out[k] = (sum over ascending i of fl(fl(x[i] w[i]) T[k][i])) norm, one accumulator from +0.0, multiply and
    add rounded separately (src/codec.rs:359-374, :480)."""
    global _tt
    T, w, norm = O.tables()
    if _tt is None:
        _tt = np.ascontiguousarray(T.T)
    tt = _tt
    with np.errstate(all="ignore"):
        x = load_rows(case, rows, mut)
        if mut == "subnormal_inputs_zero":
            x = _flush(x)
        if mut == "window_in_table":
            b, tt = x, w[:, None] * tt
        else:
            b = x * w[None, :]
        if mut == "subnormal_products_zero":
            b = _flush(b)
        if mut == "norm_in_table":
            tt = tt * norm
        order = list(range(FRAME))
        if mut == "descending_i":
            order.reverse()
        if mut == "stages_swapped":                      # the two 16-step stages on either side of the hop boundary
            order[1008:1040] = order[1024:1040] + order[1008:1024]
        s = np.full((len(rows), HOP), -0.0 if mut == "neg_zero_init" else 0.0, F32)
        s2 = np.zeros_like(s)
        for n_, i in enumerate(order):
            if mut == "fma":
                s = (b[:, i:i + 1].astype(np.float64) * tt[i][None, :].astype(np.float64) + s.astype(np.float64)).astype(F32)
                continue
            p = b[:, i:i + 1] * tt[i][None, :]
            if mut == "subnormal_products_zero":
                p = _flush(p)
            if mut == "two_accumulators" and n_ & 1:
                s2 = s2 + p
            else:
                s = s + p
        if mut == "two_accumulators":
            s = s + s2
        return s if mut == "norm_in_table" else (s * norm).astype(F32)
