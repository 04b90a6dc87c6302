"""glc_plan_crop: which frames and hops a crop [start, start + length) of a decoded clip needs (DESIGN.md section 3,
"a window of a compact blob"), held point by point to a brute-force model of the decoder's geometry:

  the decoded clip is the interleaved samples [512, 512 + len * ch) of the un-trimmed stream (the delay counts
  INTERLEAVED samples, quirk Q3); hop h is its positions [1024 ch h, 1024 ch (h + 1)); frame f contributes to hops
  f and f + 1, its 2048-sample support is the positions [1024 ch f, 1024 ch (f + 2)); the stream has n_frames
  frames and n_frames + 1 hops.

The model marks every position of the crop and asks each hop and each frame's support whether it meets one (a stream
of more than 2^20 positions is not marked: each hop is asked whether it meets the crop's interval - the same question,
hop by hop, and still no division).  Host only: no GPU is needed."""
import ctypes as C

import numpy as np
import pytest

from channel_axis_cases import CHANNELS

HOP = 1024
DELAY = 512
EINVAL = -1


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    assert hasattr(g.lib, "glc_plan_crop")
    return g


MARKED = 1 << 20                 # positions up to which a stream is marked one by one


def hops_marked(nf, per_hop, lo, hi):
    kept = np.zeros((nf + 2) * per_hop, bool)
    kept[lo:hi] = True
    assert not kept[(nf + 1) * per_hop:].any()                 # the crop lies inside the n_frames + 1 hops
    return kept.reshape(nf + 2, per_hop).any(axis=1)


def hops_by_interval(nf, per_hop, lo, hi):
    assert hi <= (nf + 1) * per_hop
    return np.array([max(lo, h * per_hop) < min(hi, (h + 1) * per_hop) for h in range(nf + 2)])


def model(nf, ch, start, length, by_hop_of=None):
    """(first_frame, n_frames, first_hop, n_hops) by marking positions."""
    per_hop = HOP * ch
    if by_hop_of is None:
        by_hop_of = hops_marked if (nf + 2) * per_hop <= MARKED else hops_by_interval
    by_hop = by_hop_of(nf, per_hop, DELAY + start * ch, DELAY + (start + length) * ch)
    hops = np.flatnonzero(by_hop)
    assert np.array_equal(hops, np.arange(hops[0], hops[-1] + 1))
    frames = [f for f in range(nf) if by_hop[f] or by_hop[f + 1]]   # support = hops f and f + 1
    assert frames == list(range(frames[0], frames[-1] + 1))
    return frames[0], len(frames), int(hops[0]), len(hops)


LENGTHS = (513, 514, 1023, 1024, 1025, 2047, 2048, 2049, 3 * HOP - 1, 3 * HOP, 3 * HOP + 1, 5 * HOP + 300)


def grid(n, ch):
    """Starts / lengths worth trying in a clip of n samples per channel: the ends, multiples of 512, and the hop
    boundaries of the un-trimmed stream for this channel count - the sample whose frame holds position 1024 ch h, for
    every hop h of the clip - with their neighbours."""
    pts = {0, 1, 2, n - 2, n - 1, n}
    for k in range(0, n + HOP, 512):
        for d in (-2, -1, 0, 1, 2):
            pts.add(k + d)
    for h in range(1, (DELAY + n * ch) // (HOP * ch) + 2):
        k = (HOP * ch * h - DELAY) // ch
        pts.update((k - 1, k, k + 1))
    for k in (171, 341, 342, 853, 854, 1195, 1196):            # inside a hop for most counts: the shortest clips have no boundary
        pts.update((k - 1, k, k + 1))
    return sorted(p for p in pts if 0 <= p <= n)


def test_the_interval_model_is_the_marking_model():
    """Where both forms of the model can run they agree: the wide channel counts are held to the same thing."""
    checked = 0
    for ch, n in ((3, 2049), (7, 1537), (17, 3 * HOP + 1)):
        nf = -(-(DELAY + n) // HOP) - 1
        pts = grid(n, ch)
        for start in pts[::2]:
            for end in pts[1::2]:
                if end > start:
                    assert model(nf, ch, start, end - start, hops_marked) == model(nf, ch, start, end - start, hops_by_interval)
                    checked += 1
    assert checked > 300


@pytest.mark.parametrize("ch", (1, 2, 3, 6) + CHANNELS + (1023, 1024, 1025))
@pytest.mark.parametrize("n", LENGTHS)
def test_plan_equals_the_brute_force_model(glc_amd, ch, n):
    g = glc_amd
    nf = g.plan_encode(n * ch, ch).n_frames
    pts = grid(n, ch)
    checked = 0
    for start in pts:
        for end in pts:
            if end <= start:
                continue
            p = g.plan_crop(n * ch, ch, start, end - start)
            got = (p.first_frame, p.n_frames, p.first_hop, p.n_hops)
            assert got == model(nf, ch, start, end - start), (ch, n, start, end - start)
            checked += 1
    assert checked > 50                                         # the grid is not empty by accident
    # the whole clip: every frame, and every hop from the one that holds position 512 on
    p = g.plan_crop(n * ch, ch, 0, n)
    assert p.first_frame == 0 and p.first_hop == 0 and p.first_frame + p.n_frames <= nf


def test_the_bare_tail_hop_has_no_frame(glc_amd):
    """The last sample of a clip lies in hop n_frames - 1 or in the bare tail hop n_frames (the second half of the
    last frame alone; a mono clip always ends there, because the delay is half a hop).  A crop of that sample needs
    the last frame only in the second case, the last two in the first."""
    g = glc_amd
    seen = set()
    for ch, n in ((1, 2 * HOP), (1, 2 * HOP + 600), (2, 2 * HOP), (2, HOP + 600), (3, 4 * HOP + 300), (6, 3 * HOP)):
        nf = g.plan_encode(n * ch, ch).n_frames
        p = g.plan_crop(n * ch, ch, n - 1, 1)
        last_hop = (DELAY + n * ch - 1) // (HOP * ch)
        assert (p.first_hop, p.n_hops) == (last_hop, 1)
        assert last_hop in (nf - 1, nf)
        if last_hop == nf:
            assert (p.first_frame, p.n_frames) == (nf - 1, 1)
        else:
            assert (p.first_frame, p.n_frames) == (nf - 2, 2)
        seen.add(last_hop == nf)
    assert seen == {True, False}


def test_refused_arguments(glc_amd):
    g = glc_amd
    L = g._lib
    n, ch = 3 * HOP, 2
    plan = L.GlcCropPlan()

    def call(ns, c, start, length, out=plan):
        crop = L.GlcCrop(start, length)
        return g.lib.glc_plan_crop(ns, c, C.byref(crop), C.byref(out) if out is not None else None)

    assert call(n * ch, ch, 0, n) == 0
    assert call(n * ch, ch, n - 1, 1) == 0
    assert call(n * ch, ch, 0, 0) == EINVAL                     # an empty crop
    assert call(n * ch, ch, n, 0) == EINVAL
    assert call(n * ch, ch, 0, n + 1) == EINVAL                 # ends behind the clip
    assert call(n * ch, ch, n, 1) == EINVAL
    assert call(n * ch, ch, 1, n) == EINVAL
    assert call(n * ch, ch, 2 ** 64 - 1, 2) == EINVAL           # start + length wraps
    assert call(n * ch, ch, 2, 2 ** 64 - 1) == EINVAL
    assert call(n * ch, 0, 0, 1) == EINVAL                      # no channels
    assert call(512 * ch, ch, 0, 1) == EINVAL                   # a clip the encoder refuses
    assert g.lib.glc_plan_crop(n * ch, ch, None, C.byref(plan)) == EINVAL
    assert call(n * ch, ch, 0, 1, out=None) == EINVAL
    with pytest.raises(g.GlcError) as e:
        g.plan_crop(n * ch, ch, 0, n + 1)
    assert e.value.code == EINVAL
    with pytest.raises(g.GlcError):
        g.plan_crop(n * ch, ch, -1, 2)
