"""Inputs for tests/test_encode_screen_drivers.py: the screened encode path under the drivers
tests/test_encode_screen_edges.py was written before - the device store encode (glc_encode_batch_device_compact and
_int), the stream push (glc_stream_enc_push_device and the host push) and glc_roundtrip_batch_device_pcm.

Every input is built twice from the same samples: as what the driver is handed (integers in their container, lanes
cut into pushes) and, in numpy, as the virtual stream the driver stages from it - a Case of encode_screen_cases whose
f0 / f1 are the frames the driver launches, so that encode_screen_edges.expected / model / screen_records decide its
rows as they decide every other case.  Nothing here loads the library but plan(), which asks glc_plan_stream_push
(host arithmetic) what a push completes: the builder does not re-derive it.

  store, round trip   encode_screen_edges.virtual_case as it stands: clip i owns nf_i + 1 slots, frames 0 .. V.
  push                V = 1 + sum (n_frames_k + 1) over the lanes that complete a frame; segment k is written from
                      sample slot_k * 1024 - 512 and holds its lane's stream from first_frame * 1024 - 512 for
                      (n_frames + 1) * 1024 samples, zeros where the stream has not begun or what the lane has received
                      ends; the frames launched are [1, V - 1).
  integers            widened as the device widens them before the oracle sees them (stream_encode_cases.widen)."""
import numpy as np

import encode_screen_edges as E
import stream_encode_cases as SC
from encode_screen_edges import F32, HOP, SR, Case
from oracle import oracle as O

S16, S32, PF32 = SC.S16, SC.S32, SC.PF32
KINDS = ("tonal", "noise", "silence", "click-first", "click-last")       # encode_screen_edges.batch_clips, in turn


def to_container(x, fmt, bits):
    """Float samples as the driver is handed them -> (samples in their container, the float32 samples the device makes
    of them).  A click of 2.0 clips to full scale: it is a click all the same."""
    if fmt == PF32:
        x = np.ascontiguousarray(x, F32)
        return x, x
    xi = SC.to_int(np.asarray(x, np.float64), fmt, bits)
    return xi, SC.widen(xi, bits)


class Input:
    """One driver input.  clips: per clip or lane the interleaved samples in their container; wide: the same as the
    float32 the device widens them to - what the oracle encodes; case: the rows the driver launches; segs: per slot
    of the virtual stream (first frame of the slot counted from case.f0, frames, the clip's or lane's first frame there,
    frames of the whole clip or stream, content kind, clip or lane)."""

    def __init__(self, name, driver, ch, fmt, bits, planar, off, clips, wide, case, segs):
        self.name, self.driver, self.ch, self.fmt, self.bits, self.planar, self.off = name, driver, ch, fmt, bits, planar, off
        self.clips, self.wide, self.case, self.segs = clips, wide, case, segs

    @property
    def rows(self):
        return self.case.M

    def real_frames(self):
        """Frames of the case (from f0) that some clip or lane owns: every one but the junk frames."""
        own = np.zeros(self.case.f1 - self.case.f0, bool)
        for at, n, *_ in self.segs:
            own[at:at + n] = True
        return own


# ---------------------------------------------------------------------------------------------------- store, round trip

def batch_input(name, driver, ch, fmt, bits, planar, off, floats):
    pairs = [to_container(x, fmt, bits) for x in floats]
    wide = [w for _, w in pairs]
    c = E.virtual_case(name, SR, ch, wide)
    segs = [(at, n, 0, n, KINDS[i % 5], i) for i, (at, n) in enumerate(c.slots)]
    return Input(name, driver, ch, fmt, bits, planar, off, [p for p, _ in pairs], wide, c, segs)


def store_inputs():
    stereo = E.encode_batch_clips()                                       # 20 stereo clips of 5..9 frames: V = 160, 320 rows
    return [
        batch_input("store-f32", "store", 2, PF32, 32, True, 1, stereo),            # planar: planes 3 samples apart from the longest clip
        batch_input("store-s16", "store", 2, S16, 16, False, 3, stereo),
        batch_input("store-ch8", "store", 8, PF32, 32, True, 2, E.batch_clips(SR, 8, 6, (5, 6, 7), seed=83)),     # V = 42, 336 rows
        batch_input("store-ch3", "store", 3, PF32, 32, False, 1, E.batch_clips(SR, 3, 10, (8, 9), seed=57)),      # V = 95, 285 rows
    ]


def roundtrip_inputs():
    return [batch_input("rtpcm-s16", "rtpcm", 2, S16, 16, True, 1, E.batch_clips(SR, 2, 14, (8, 9, 10), seed=31))]   # V = 139, 278 rows


# ---------------------------------------------------------------------------------------------------- push

def plan(received, n_new, finish):
    """(first_frame, n_frames) of a push: glc_plan_stream_push's answer."""
    import glc_amd
    p = glc_amd.plan_stream_push(int(received), int(n_new), bool(finish))
    return int(p.first_frame), int(p.n_frames)


def push_case(name, ch, lanes, received, n_new, finish):
    """The virtual stream of ONE push and the segments the library reports for it.  lanes[i]: the float32 stream of lane
    i as the device widens it, interleaved; received / n_new / finish per lane.
    -> (Case of frames [1, V - 1), [(lane, first_frame, n_frames)], [(slot - 1, n_frames)])."""
    segs = []
    for i in range(len(lanes)):
        if n_new[i] or finish[i]:
            f0, nf = plan(received[i], n_new[i], finish[i])
            if nf:
                segs.append((i, f0, nf))
    V = 1 + sum(nf + 1 for _, _, nf in segs)
    vs = np.zeros((V * HOP, ch), F32)
    slot, slots = 1, []
    for lane, f0, nf in segs:
        x = lanes[lane].reshape(-1, ch)
        end = received[lane] + n_new[lane]
        assert end <= x.shape[0]
        x0, n = f0 * HOP - HOP // 2, (nf + 1) * HOP
        lo, hi = max(x0, 0), min(x0 + n, end)
        dst = slot * HOP - HOP // 2
        vs[dst + lo - x0:dst + hi - x0] = x[lo:hi]
        slots.append((slot - 1, nf))
        slot += nf + 1
    assert slot == V
    return Case(name, "drivers", SR, ch, vs, 1, V - 1), segs, slots


class Session:
    """The pushes of one streaming session: lane i's stream and the samples per channel each push hands it, the last of
    which finishes it (the schedule of tests/test_stream_encode.py).  inputs(): one Input per push, named by `names`
    (None: the push is part of the session and no input of its own - it completes too little to matter)."""

    def __init__(self, tag, ch, fmt, bits, planar, off, floats, kinds, sizes, names):
        self.tag, self.ch, self.fmt, self.bits, self.planar, self.off = tag, ch, fmt, bits, planar, off
        pairs = [to_container(x, fmt, bits) for x in floats]
        self.clips, self.wide, self.kinds, self.sizes, self.names = [p for p, _ in pairs], [w for _, w in pairs], kinds, sizes, names
        self.frames = [O.num_frames(w.size, ch) for w in self.wide]
        for w, s in zip(self.wide, sizes):
            assert sum(s) == w.size // ch

    def lanes(self):
        """As test_stream_encode.schedule takes them: per lane [(stream in its container, sizes)]."""
        return [[(x, list(s))] for x, s in zip(self.clips, self.sizes)]

    def pushes(self):
        """Per push (received, n_new, finish) per lane; a lane whose sizes have run out receives nothing."""
        n_push = max(len(s) for s in self.sizes)
        out = []
        for k in range(n_push):
            rec = [sum(s[:k]) if k < len(s) else 0 for s in self.sizes]
            new = [s[k] if k < len(s) else 0 for s in self.sizes]
            fin = [k == len(s) - 1 for s in self.sizes]
            out.append((rec, new, fin))
        return out

    def inputs(self):
        out = []
        for k, (rec, new, fin) in enumerate(self.pushes()):
            name = self.names[k] if k < len(self.names) else None
            if name is None:
                continue
            c, segs, slots = push_case(name, self.ch, self.wide, rec, new, fin)
            info = [(at, n, f0, self.frames[lane], self.kinds[lane], lane) for (lane, f0, n), (at, _) in zip(segs, slots)]
            inp = Input(name, "push", self.ch, self.fmt, self.bits, self.planar, self.off, self.clips, self.wide, c, info)
            inp.push, inp.session = k, self
            out.append(inp)
        return out


def _done(frames, jitter):
    """Samples per channel after which exactly `frames` frames of a stream are final, `jitter` past the first such count."""
    assert 0 <= jitter < HOP
    return HOP * (frames - 1) + 3 * HOP // 2 + jitter


def session_main(tag, fmt, bits, planar, off):
    """8 stereo lanes of 70-frame streams in four pushes that complete frames 0..19, 20..39, 40..48 and 49..69 (the last
    finishes): 334, 334, 158 and 350 rows.  The third is under the 256-row threshold and over the matrix form's 128."""
    floats = E.batch_clips(SR, 2, 8, (70,), seed=11)
    sizes = []
    for i, x in enumerate(floats):
        cuts = [0, _done(20, 37 * i), _done(40, 100 * i), _done(49, 1000 - 90 * i), x.size // 2]
        sizes.append([b - a for a, b in zip(cuts, cuts[1:])])
    sfx = "" if fmt == PF32 else "-s32"
    return Session(tag, 2, fmt, bits, planar, off, floats, [KINDS[i % 5] for i in range(8)], sizes,
                   [f"push-first{sfx}", f"push-middle{sfx}", f"push-gap{sfx}", f"push-finish{sfx}"])


def session_ragged():
    """9 stereo lanes, one push that counts and a second that only ends the streams: lanes 1 and 6 get nothing in the
    first, lanes 3 and 7 too little to complete a frame (700 and 1535 samples: held back only), lane 4 finishes a
    5-frame stream, lanes 0, 2, 5 and 8 complete 30 frames of 32: V = 1 + 4 * 31 + 6 = 131, 258 rows."""
    long = E.batch_clips(SR, 2, 4, (32,), seed=23)                        # tonal, noise, silence, click-first
    short = E.batch_clips(SR, 2, 5, (3, 5), seed=29)                      # 3, 5, 3, 5, 3 frames: tonal, noise, silence, click-first, click-last
    floats = [long[0], short[0], long[1], short[2], short[3], long[2], short[4], short[1], long[3]]
    kinds = ["tonal", "tonal", "noise", "silence", "click-first", "silence", "click-last", "noise", "click-first"]
    sizes = []
    for i, x in enumerate(floats):
        L = x.size // 2
        first = {1: 0, 6: 0, 3: 700, 7: 1535, 4: L}.get(i, _done(30, 111 * i))
        sizes.append([L] if first == L else [first, L - first])
    return Session("ragged", 2, PF32, 32, False, 1, floats, kinds, sizes, ["push-ragged", None])


def session_ch4():
    """4 lanes of 4 channels, 16-frame streams finished by their one push: V = 69, 268 rows."""
    floats = E.batch_clips(SR, 4, 4, (16,), seed=41)
    return Session("ch4", 4, PF32, 32, True, 2, floats, [KINDS[i] for i in range(4)], [[x.size // 4] for x in floats], ["push-ch4"])


def session_small():
    """Two stereo lanes completing 10 frames each: 42 rows, under every threshold."""
    floats = E.batch_clips(SR, 2, 2, (10,), seed=43)
    return Session("small", 2, PF32, 32, True, 0, floats, [KINDS[0], KINDS[1]], [[x.size // 2] for x in floats], ["push-small"])


_sessions = {}


def sessions():
    if not _sessions:
        for s in (session_main("main-f32", PF32, 32, True, 1), session_main("main-s32", S32, 24, False, 1), session_ragged(),
                  session_ch4(), session_small()):
            _sessions[s.tag] = s
    return _sessions


_inputs = {}


def inputs():
    """name -> Input, built once."""
    if not _inputs:
        for inp in store_inputs() + roundtrip_inputs() + [i for s in sessions().values() for i in s.inputs()]:
            _inputs[inp.name] = inp
    return _inputs


# ---------------------------------------------------------------------------------------------------- the lng round

LNG_FRAMES, LNG_CHUNK, LNG_CLICKS = 4096 + 300, 4096, (2000, 4096 + 150)


def lng_clip():
    """One tonal stereo clip of one full chunk plus 300 frames, a click far inside each chunk."""
    x = E.stream(SR, 2, LNG_FRAMES)[:LNG_FRAMES * HOP - 300]
    for f in LNG_CLICKS:
        E._click(x, f)
    x = np.ascontiguousarray(x, F32).reshape(-1)
    assert O.num_frames(x.size, 2) == LNG_FRAMES
    return x
