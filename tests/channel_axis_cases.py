"""Cases for tests/test_channel_axis.py: the batch, store and crop paths across the channel axis.  The clip pool with its
oracle values, the strided layouts, the crops, and a numpy model of "what a batch call writes where" with the slips it
is mutated with.  Nothing here touches the GPU.

Expected values come from outside the code under test: streams and samples from the CPU oracle, the blob of a store
from the host twins (glc_compact_records on the oracle's records for what the ENCODER stores, glc_frames_to_compact on
the oracle's stream for what a host uploads), crops as slices of the oracle's whole-clip decode, the planner's records
from store_draw_cases.plan_model, the 16-bit narrowing from test_int_pcm's restatement.

The model (`writes`, `slots`, `clip_rows`) is symbolic: it says which position of the un-trimmed stream lands at which
element of the output, and never asks the oracle, so the coverage conditions and the power test cost nothing.
"""
from __future__ import annotations

import numpy as np

import conftest as cf
import crop_cases as CC
import roundtrip_cases as RC
import store_draw_cases as S
from conftest import O

SR = 44100
HOP, FRAME, DELAY = RC.HOP, RC.FRAME, CC.DELAY
F32 = np.float32
NAN_BITS = CC.NAN_BITS
I16_PATTERN = 0x7ABC

# The channel counts, and what each is there for (512 % ch is where in a sample frame a crop begins, quirk Q3):
CHANNELS = (
    4,      # the specialised staging (k_stage_clips_planar<4>) and D2 (CH = 4) instantiations; 512 % 4 == 0
    5,      # odd: the generic paths; 512 % 5 == 2, a sample frame straddles a hop boundary
    7,      # odd; 512 % 7 == 1, the one residue at which an off-by-one in the slot formula shows
    9,      # the first count beyond every specialisation; 512 % 9 == 8
    16,     # a power of two with NO specialisation: it must take the dividing path; 512 % 16 == 0
    17,     # prime; 512 % 17 == 2
    257,    # above 256: K1's path of its own, ch as a grid dimension of staging and planar D2; 512 % 257 == 255
    513,    # the delay is shorter than one sample frame: position 512 is channel 512 of time 0; 512 % 513 == 512
)
OLD = (1, 2, 3, 6, 8)            # what the batch, store and crop suites ran before
WIDE = 17                        # above this the pool is the two short clips


def is_wide(ch):
    return ch > WIDE


# ------------------------------------------------------------------------------------------ the pool

SMALL_LENGTHS = (513, 1024, 1535, 1537, 2049)    # one to three hops, on both sides of the length that adds a frame
WIDE_LENGTHS = (513, 1537)                       # one and two frames


def names(ch):
    if is_wide(ch):
        return tuple(f"chord{n}" for n in WIDE_LENGTHS)
    return tuple(f"chord{n}" for n in SMALL_LENGTHS) + ("mixed",)


def signal(ch, name):
    if name == "mixed":          # chord, LCG noise, chord: both frame kinds, a raw frame next to a compressed one
        return RC.mixed_clip(SR, ch)
    n = int(name[5:])
    return RC.chord(SR, ch, n, seed=100 + n % 97)


class Item:
    """One clip of the pool; every oracle value is computed on first use and kept."""

    def __init__(self, ch, name):
        self.ch, self.name = ch, name
        self._c = {}

    def _get(self, key, make):
        if key not in self._c:
            self._c[key] = make()
        return self._c[key]

    @property
    def x(self):
        return self._get("x", lambda: np.ascontiguousarray(signal(self.ch, self.name), F32))

    @property
    def n(self):
        return self.x.size

    @property
    def pc(self):
        return self.x.size // self.ch

    @property
    def nf(self):
        return RC.frames_of(self.pc)

    @property
    def glc(self):
        return self._get("glc", lambda: O.encode(self.x, SR, self.ch).glc)

    @property
    def dec(self):
        def make():
            d = O.decode(self.glc)[0]
            assert d.size == self.n
            return d
        return self._get("dec", make)

    @property
    def dec16(self):
        import test_int_pcm
        return self._get("dec16", lambda: test_int_pcm.narrow(self.dec))

    @property
    def raw(self):
        """Per frame: is it a raw frame of the oracle's stream."""
        return self._get("raw", lambda: [f["raw"] is not None for f in cf.parse_glc(self.glc)["frames"]])

    @property
    def records(self):
        return self._get("records", lambda: O.encode_range_records(self.x, 0, self.pc, self.n, SR, self.ch, 0, self.nf, taps=True)[0])

    @property
    def blob_enc(self):
        """The blob the ENCODER's store holds: the host twin of the packing on the oracle's records."""
        import glc_amd as g
        return self._get("blob_enc", lambda: np.ascontiguousarray(g.compact_records(self.records, self.ch), np.uint8))

    @property
    def blob(self):
        """The blob of the oracle's stream (glc_frames_to_compact): what a host uploads into a store."""
        def make():
            import glc_amd as g
            return np.frombuffer(g.frames_to_compact(g.EncodedAudio.from_bytes(self.glc)), np.uint8).copy()
        return self._get("blob", make)


_items = {}


def item(ch, name):
    if (ch, name) not in _items:
        _items[(ch, name)] = Item(ch, name)
    return _items[(ch, name)]


def pool(ch):
    return [item(ch, n) for n in names(ch)]


def batch_names(ch):
    """The clips of a batch call: the ragged pool; the two wide clips twice, so that four clips start in a layout."""
    return names(ch) * 2 if is_wide(ch) else names(ch)


def pool_lengths(ch):
    """Samples per channel of batch_names(ch), without making a signal."""
    return [17 * HOP + 300 if n == "mixed" else int(n[5:]) for n in batch_names(ch)]


# ------------------------------------------------------------------------------------------ layouts

def odd_up(v):
    return v + 1 if v % 2 == 0 else v + 2


def layout_kw(ch, T, planar, tail=5):
    """Batch arguments of roundtrip_batch's helper: lead = 1 and odd strides with gaps, so that with an odd stride the
    planes (planar) and the clips start at every offset from a 16-byte boundary in turn."""
    if planar:
        cs = odd_up(T)
        return dict(lead=1, tail=tail, channel_stride=cs, clip_stride=odd_up((ch - 1) * cs + T))
    return dict(lead=1, tail=tail, clip_stride=odd_up(T * ch))


def start_offsets(ch, n_clips, T, planar):
    """Element offsets modulo 4 (16 bytes) of every run a staging or D2 kernel starts: clips, and planes when planar."""
    kw = layout_kw(ch, T, planar)
    out = set()
    for i in range(n_clips):
        at = kw["lead"] + i * kw["clip_stride"]
        for c in range(ch if planar else 1):
            out.add((at + c * kw.get("channel_stride", 0)) % 4)
    return out


# ------------------------------------------------------------------------------------------ crops

CROP_LENGTHS = (1, 1024, 1025)
WIDE_DRAW_LENGTHS = (1, 2)


def last_start_of_hop(h, ch):
    """The per-channel sample whose frame begins at the last position of hop h a sample frame can begin at,
    1024 ch (h + 1) - ch + 512 % ch: the frame that holds the boundary to hop h + 1 when 512 % ch != 0, else the last
    frame wholly in front of it."""
    at = HOP * ch * (h + 1) - ch + DELAY % ch
    assert (at - DELAY) % ch == 0
    return (at - DELAY) // ch


def straddler(n, ch):
    """(start, length): two sample frames from the last start of hop 0 - across the first hop boundary of the
    un-trimmed stream, the boundary inside the first of them when 512 % ch != 0."""
    b = last_start_of_hop(0, ch)
    assert 1 <= b and b + 2 <= n
    return b, 2


def crops(ch, name):
    """(start, length) crops of a pool clip.  Wide counts: the first sample and the frames around the only hop boundary
    (a one-frame clip lies inside hop 0: its last sample instead).  Else every edge crop_cases and store_draw_cases
    name, and lengths 1, 1024, 1025 at every boundary start; whole-clip-sized windows of the long mixed clip are left to
    the batch decode."""
    n = 17 * HOP + 300 if name == "mixed" else int(name[5:])
    nf = RC.frames_of(n)
    if is_wide(ch):
        return [(0, 1), straddler(n, ch) if CC.hop_of(n - 1, ch - 1, ch) >= 1 else (n - 1, 1)]
    w = set(CC.edge_windows(n, ch, nf)) | set(S.edge_draws(n, ch, nf))
    for length in CROP_LENGTHS:
        w |= {(s, length) for s in S.boundary_starts(n, ch, length)}
    if name == "mixed":
        w = {x for x in w if x[1] <= 1025} | {(0, n)}
    return sorted(w)


def draws(ch, length):
    """(clip index into names(ch), start) selections of one store draw of `length`: every boundary start of every clip."""
    out = []
    for e, name in enumerate(names(ch)):
        n = 17 * HOP + 300 if name == "mixed" else int(name[5:])
        if is_wide(ch):
            pts = sorted({c[0] for c in crops(ch, name) if c[1] == length} | {0, n - length})
        else:
            pts = S.boundary_starts(n, ch, length)
        out += [(e, s) for s in pts]
    return out


def tables_of_blob(blob, ch):
    """row_begin, row_cnt, row_raw of a VALID blob, as compact_decode_cases.tables gives them for a description."""
    import struct

    import compact_decode_cases as K
    magic, bch, nf, n_pairs, _, nbytes = struct.unpack_from("<IIQQQQ", blob.tobytes(), 0)
    assert magic == K.MAGIC and nbytes == blob.size
    assert bch == ch
    m = nf * ch
    o_israw, o_scale, o_cnt, o_pairs, _ = K.layout(ch, nf)
    is_raw = np.repeat(blob[o_israw:o_israw + nf].astype(bool), ch)
    cnt = blob[o_cnt:o_cnt + 4 * m].view(np.uint32).copy()
    assert int(cnt.sum(dtype=np.uint64)) == n_pairs and not cnt[is_raw].any()
    excl = np.concatenate([[0], np.cumsum(cnt.astype(np.uint64))[:-1]]).astype(np.uint64)
    raw_off = K.align64(o_pairs + 4 * n_pairs)
    begin = np.where(is_raw, 0, o_pairs // 4 + excl).astype(np.uint64)
    planes_before = np.concatenate([[0], np.cumsum(is_raw)[:-1]]).astype(np.int64)
    first_plane = planes_before - (np.arange(m) % ch)
    row_raw = np.where(is_raw, raw_off // 2 + first_plane * FRAME, -1).astype(np.int64)
    return begin, cnt, row_raw


# ------------------------------------------------------------------------------------------ the model

# One edit each.  The first five are the slips as they are usually named; every one of them already changes something at
# 3 and 6 channels (a sample frame straddles there too, and 3 and 6 are no powers of two) or at 2, so the old suites
# could see them - SEEN_BEFORE says where, from the arithmetic and not from a run.  The five behind them are the same
# slips in the form only the new counts can show: each changes NOTHING at 1, 2, 3, 6 and 8.
LITERAL = ("delay_per_channel", "planes_start_together", "shift_and_mask_of_next_pow2", "slots_without_residue", "clip_table_in_frames")
SEEN_BEFORE = {
    "delay_per_channel": {2, 3, 6, 8},             # 512 * ch != 512 unless ch == 1
    "planes_start_together": {3, 6},               # planes differ exactly where 512 % ch != 0
    "shift_and_mask_of_next_pow2": {3, 6},         # exact for a power of two
    "slots_without_residue": {3, 6},               # the term is 0 where ch divides 512
    "clip_table_in_frames": {2, 3, 6, 8},          # rows == frames only for mono
}
NEW_ONLY = (
    "delay_at_least_a_frame",        # the delay thought of per channel: no channel loses less than one sample -> max(512, ch)
    "plane_index_in_8_bits",         # the plane whose start time is computed is c & 255: planes from 256 on start with plane c - 256
    "pow2_takes_the_widest_shift",   # every power of two above 8 is given the CH = 8 instantiation (o >> 3, o & 7)
    "slot_residue_exclusive",        # the last position a start can take counted one short: 512 % ch - 1 (shows where 512 % ch == 1)
    "hop_index_in_16_bits",          # the interleaved index inside a hop kept in 16 bits: wraps where 1024 * ch > 65536
)
MUTATIONS = LITERAL + NEW_ONLY


def next_pow2(v):
    p = 1
    while p < v:
        p *= 2
    return p


def delay_of(ch, mut=None):
    if mut == "delay_per_channel":
        return DELAY * ch
    if mut == "delay_at_least_a_frame":
        return max(DELAY, ch)
    return DELAY


def split(o, ch, mut=None):
    """(time, channel) inside a hop's blocks of its interleaved index o (an array)."""
    if mut == "hop_index_in_16_bits":
        o = o & 0xFFFF
    if mut == "shift_and_mask_of_next_pow2":
        p = next_pow2(ch)
        return o >> (p.bit_length() - 1), o & (p - 1)
    if mut == "pow2_takes_the_widest_shift" and ch > 8 and ch & (ch - 1) == 0:
        return o >> 3, o & 7
    return o // ch, o % ch


def slots(length, ch, mut=None):
    per_hop = HOP * ch
    r = DELAY % ch
    if mut == "slots_without_residue":
        r = 0
    if mut == "slot_residue_exclusive":
        r = max(r - 1, 0)
    hops = (per_hop - ch + r + length * ch - 1) // per_hop + 1
    return hops, hops + 1


def clip_rows(ch, clip_frames, mut=None):
    """[first table row, rows) of every clip of a virtual record stream with one junk record behind each clip."""
    unit = 1 if mut == "clip_table_in_frames" else ch
    out, slot = [], 0
    for nf in clip_frames:
        out.append((slot * unit, nf * unit))
        slot += nf + 1
    return out


def writes(ch, n, start, length, planar, dst=0, cstride=0, mut=None):
    """Which position of the un-trimmed stream lands at which output element when samples [start, start + length) per
    channel of a clip of n are decoded to element `dst` on (planes `cstride` apart when planar): the trim, one
    descriptor per hop as hop_desc states it, and the placement of k_overlap_add_strided / k_overlap_add_planar.
    -> (element offsets ascending, stream position + 1 of each; 0 where an element is written twice or read from
    behind the 1024 times a hop's blocks hold).  A position is hop * 1024 ch + time * ch + channel."""
    per_hop = HOP * ch
    t0 = delay_of(ch, mut) + start * ch
    span = length * ch
    h0, h1 = t0 // per_hop, (t0 + span - 1) // per_hop
    addr, src = [], []
    planes = planar and ch > 1
    for h in range(h0, h1 + 1):
        lo, hi = max(t0, h * per_hop), min(t0 + span, (h + 1) * per_hop)
        j0, first, cnt = lo - t0, lo - h * per_hop, hi - lo
        if not planes:
            k = np.arange(cnt, dtype=np.int64)
            i, c = split(first + k, ch, mut)
            addr.append(dst + j0 + k)
            src.append(np.where(i < HOP, h * per_hop + i * ch + c, -1))      # a block holds 1024 times of a hop
            continue
        c = np.arange(ch, dtype=np.int64)
        cs = c & 0xFF if mut == "plane_index_in_8_bits" else c
        j1 = j0 + cnt
        c_lo = np.zeros_like(c) if mut == "planes_start_together" else cs
        t_lo = np.where(j0 > c_lo, (j0 - c_lo + ch - 1) // ch, 0)
        t_hi = np.where(j1 > cs, (j1 - cs + ch - 1) // ch, 0)
        cnt_c = np.maximum(t_hi - t_lo, 0)
        o0 = first + t_lo * ch + c - j0
        i0, cc = split(o0, ch, mut)
        rep = np.repeat(c, cnt_c)
        k = np.arange(int(cnt_c.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt_c) - cnt_c, cnt_c)
        addr.append(dst + rep * cstride + t_lo[rep] + k)
        src.append(np.where(i0[rep] + k < HOP, h * per_hop + (i0[rep] + k) * ch + cc[rep], -1))
    addr, src = np.concatenate(addr), np.concatenate(src) + 1
    order = np.argsort(addr, kind="stable")
    addr, src = addr[order], src[order]
    twice = np.flatnonzero(addr[1:] == addr[:-1])
    if twice.size:
        src[twice] = 0
        keep = np.ones(addr.size, bool)
        keep[twice + 1] = False
        addr, src = addr[keep], src[keep]
    return addr, src


def closed_form(ch, n, start, length, planar, dst=0, cstride=0):
    """What `writes` must give, from the definition alone: sample t of channel c is position 512 + t * ch + c."""
    t, c = np.meshgrid(np.arange(start, start + length, dtype=np.int64), np.arange(ch, dtype=np.int64), indexing="ij")
    pos = DELAY + t * ch + c + 1
    at = dst + c * cstride + (t - start) if planar and ch > 1 else dst + (t - start) * ch + c
    order = np.argsort(at.reshape(-1), kind="stable")
    return at.reshape(-1)[order], pos.reshape(-1)[order]


def model_cases(ch):
    """(n, start, length, planar) the power test evaluates per channel count: whole clips, the frames around every hop
    boundary of a three-hop clip, single samples there, and 1025 samples from the last start of a hop."""
    out = []
    for planar in (True, False):
        out.append((513, 0, 513, planar))
        n = 1537
        s, l = straddler(n, ch)
        out += [(n, 0, 1, planar), (n, s, l, planar), (n, s + 1, 1, planar), (n, s, 1, planar), (n, s - 1, 3, planar)]
        if not is_wide(ch):
            out.append((n, 0, n, planar))
            n = 2 * HOP + 600
            for b in (CC.boundary_sample(1, ch), CC.boundary_sample(2, ch)):
                out += [(n, b, 1, planar), (n, b - 1, 2, planar), (n, max(b - 1024, 0), 1025, planar)]
    return out


def outcome(ch, mut=None):
    """Everything the model says about a channel count, comparable with ==."""
    got = []
    for n, start, length, planar in model_cases(ch):
        a, s = writes(ch, n, start, length, planar, dst=3, cstride=odd_up(length), mut=mut)
        got.append((a.tobytes(), s.tobytes()))
    got.append(tuple(slots(length, ch, mut) for length in (1, 2, 1023, 1024, 1025, 2048, 2049)))
    got.append(tuple(clip_rows(ch, (3, 1, 2), mut)))
    return got
