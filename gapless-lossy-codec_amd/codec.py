"""Host-side mirror of the reference's codec API (src/codec.rs) over the C ABI (include/glc.h).

Names, argument meaning and results follow the reference crate:

    Encoder::new(sample_rate)                      src/codec.rs:406   -> Encoder(sample_rate)
    Encoder::encode(&samples, channels)            src/codec.rs:421   -> Encoder.encode(samples, channels)
    Decoder::new(channels, sample_rate)            src/codec.rs:581   -> Decoder(channels, sample_rate)
    Decoder::decode(&encoded, progress)            src/codec.rs:744   -> Decoder.decode(encoded)
    Decoder::decode_streaming(encoded, progress)   src/codec.rs:595   -> Decoder.decode_streaming(encoded)
    save_encoded / load_encoded                    src/codec.rs:774-786

The reference panics on degenerate input; here those cases raise GlcError with
code GLC_EINVAL.  All arithmetic happens in libglc_hip.so on a gfx950 device; this module holds no
numerics and no fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np

from ._lib import (FRAMES_HOOK, GLC_EINVAL, GLC_PCM_F32, GLC_PCM_S16, GLC_PCM_S32, GlcClipLayout, GlcCompactInfo, GlcCompactStatus, GlcCrop, GlcCropPlan, GlcError,
                   GlcFramesGather, GlcFramesView, GlcInfo, GlcPlan, GlcRoundtripInfo, GlcStreamDecPlan, GlcStoreCut, GlcStreamPushPlan, GlcStreamSeg, check, lib)

FRAME_SIZE = 2048        # src/codec.rs:15
HOP_SIZE = 1024          # src/codec.rs:16
FRAMES_PER_CHUNK = 500   # src/codec.rs:18


@dataclass
class AudioHeader:  # src/codec.rs:39-45
    sample_rate: int
    channels: int
    total_samples: int


@dataclass
class GaplessInfo:  # src/codec.rs:47-53
    encoder_delay: int
    padding: int
    original_length: int


@dataclass
class EncodedFrame:  # src/codec.rs:56-69
    sparse_coeffs_per_channel: List[List[Tuple[int, int]]]
    scale_factors: List[float]
    raw_pcm: Optional[np.ndarray]


@dataclass
class AudioChunk:  # src/codec.rs:81-85
    samples: np.ndarray
    is_last: bool


class _Frames(Sequence):
    """Lazy `Vec<EncodedFrame>` view over a glc_frames handle."""

    def __init__(self, owner: "EncodedAudio"):
        self._o = owner

    def __len__(self) -> int:
        return self._o.info().n_frames

    def __getitem__(self, f):
        if isinstance(f, slice):
            return [self[i] for i in range(*f.indices(len(self)))]
        n = len(self)
        if f < 0:
            f += n
        if not 0 <= f < n:
            raise IndexError(f)
        h = self._o._h
        if lib.glc_frame_is_raw(h, f) == 1:
            ln = C.c_uint64()
            check(lib.glc_frame_raw(h, f, None, 0, C.byref(ln)))
            raw = np.empty(ln.value, np.int16)
            check(lib.glc_frame_raw(h, f, raw.ctypes.data_as(C.c_void_p), ln.value, C.byref(ln)))
            return EncodedFrame([], [], raw)
        lists, scales = [], []
        c = 0
        while True:
            n_pairs = C.c_uint32()
            if lib.glc_frame_sparse(h, f, c, None, None, 0, C.byref(n_pairs)) != 0:
                break
            idx = np.empty(n_pairs.value, np.uint16)
            q = np.empty(n_pairs.value, np.int16)
            check(lib.glc_frame_sparse(h, f, c, idx.ctypes.data_as(C.c_void_p),
                                       q.ctypes.data_as(C.c_void_p), n_pairs.value, C.byref(n_pairs)))
            lists.append(list(zip(idx.tolist(), q.tolist())))
            c += 1
        c = 0
        while True:
            s = C.c_float()
            if lib.glc_frame_scale(h, f, c, C.byref(s)) != 0:
                break
            scales.append(s.value)
            c += 1
        return EncodedFrame(lists, scales, None)


class EncodedAudio:
    """src/codec.rs:31-37; owns a library-side glc_frames object."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.glc_frames_free(h)

    def info(self) -> GlcInfo:
        i = GlcInfo()
        check(lib.glc_frames_info(self._h, C.byref(i)))
        return i

    @property
    def header(self) -> AudioHeader:
        i = self.info()
        return AudioHeader(i.sample_rate, i.channels, i.total_samples)

    @property
    def gapless_info(self) -> GaplessInfo:
        i = self.info()
        return GaplessInfo(i.encoder_delay, i.padding, i.original_length)

    @property
    def frames(self) -> _Frames:
        return _Frames(self)

    def to_bytes(self) -> bytes:
        """bincode::serialize(encoded) — the .glc byte stream (src/codec.rs:776)."""
        n = lib.glc_serialized_size(self._h)
        buf = (C.c_uint8 * n)()
        w = C.c_uint64()
        check(lib.glc_serialize(self._h, buf, n, C.byref(w)))
        return bytes(buf)

    @staticmethod
    def from_bytes(data: bytes) -> "EncodedAudio":
        """bincode::deserialize (src/codec.rs:784)."""
        arr = np.frombuffer(data, np.uint8)
        out = C.c_void_p()
        check(lib.glc_deserialize(arr.ctypes.data_as(C.c_void_p), arr.size, C.byref(out)))
        return EncodedAudio(out.value)

    # ---- the structured bridge (include/glc.h glc_frames_view): EncodedAudio as flat arrays ----------
    _PART_TYPES = (("list_begin", np.uint64), ("list_off", np.uint64), ("pairs", np.uint32), ("scale_begin", np.uint64),
                   ("scales", np.float32), ("raw_tag", np.uint8), ("raw_begin", np.uint64), ("raw", np.int16))

    @property
    def stream_id(self) -> int:
        return int(lib.glc_frames_stream_id(self._h))

    def parts(self) -> dict:
        """Copies of the flat pools behind this EncodedAudio (glc_frames_get_view): header fields plus
        list_begin / list_off / pairs / scale_begin / scales / raw_tag / raw_begin / raw as numpy arrays."""
        v = GlcFramesView()
        check(lib.glc_frames_get_view(self._h, C.byref(v)))
        return _view_to_dict(v)

    @staticmethod
    def from_parts(parts: dict, stream_id: int = 0) -> "EncodedAudio":
        """glc_frames_from_parts: the inverse of parts(); offsets are validated by the library."""
        keep = {k: np.ascontiguousarray(parts[k], t).reshape(-1) for k, t in EncodedAudio._PART_TYPES}
        v = GlcFramesView()
        for k in ("sample_rate", "channels", "total_samples", "encoder_delay", "padding", "original_length"):
            setattr(v, k, int(parts[k]))
        v.n_frames = int(parts.get("n_frames", keep["raw_tag"].size))
        v.n_lists = int(parts.get("n_lists", max(keep["list_off"].size, 1) - 1))
        v.n_pairs = int(parts.get("n_pairs", keep["pairs"].size))
        v.n_scales = int(parts.get("n_scales", keep["scales"].size))
        v.n_raw = int(parts.get("n_raw", keep["raw"].size))
        for k, _ in EncodedAudio._PART_TYPES:
            setattr(v, k, keep[k].ctypes.data if keep[k].size else None)
        out = C.c_void_p()
        check(lib.glc_frames_from_parts(C.byref(v), stream_id, C.byref(out)))
        return EncodedAudio(out.value)

    @staticmethod
    def from_nested(header: AudioHeader, frames, gapless: GaplessInfo, stream_id: int = 0) -> "EncodedAudio":
        """glc_frames_from_gather from the reference's nested shape: `frames` is a sequence of
        (sparse_coeffs_per_channel: list of uint32 arrays of packed (idx | q << 16) pairs,
         scale_factors: float32 array, raw_pcm: int16 array or None) - one pointer per vector crosses."""
        lists_per, list_ptr, list_len, scales_per, scale_ptr, raw_ptr, raw_len, keep = [], [], [], [], [], [], [], []
        for lists, scales, raw in frames:
            lists_per.append(len(lists))
            for l in lists:
                a = np.ascontiguousarray(l, np.uint32).reshape(-1)
                keep.append(a)
                list_ptr.append(a.ctypes.data if a.size else 0)
                list_len.append(a.size)
            sc = np.ascontiguousarray(scales, np.float32).reshape(-1)
            keep.append(sc)
            scales_per.append(sc.size)
            scale_ptr.append(sc.ctypes.data if sc.size else 0)
            if raw is None:
                raw_ptr.append(0)
                raw_len.append(0)
            else:
                r = np.ascontiguousarray(raw, np.int16).reshape(-1)
                n_r = r.size
                if n_r == 0:
                    r = np.zeros(1, np.int16)  # Some(vec![]): a non-null pointer with length 0
                keep.append(r)
                raw_ptr.append(r.ctypes.data)
                raw_len.append(n_r)
        arr = lambda x, t: np.ascontiguousarray(np.array(x, dtype=t))
        a_lp, a_ll, a_sp = arr(lists_per, np.uint32), arr(list_len, np.uint32), arr(scales_per, np.uint32)
        a_ptr, a_sptr, a_rptr, a_rl = arr(list_ptr, np.uint64), arr(scale_ptr, np.uint64), arr(raw_ptr, np.uint64), arr(raw_len, np.uint64)
        g = GlcFramesGather()
        g.sample_rate, g.channels, g.total_samples = header.sample_rate, header.channels, header.total_samples
        g.encoder_delay, g.padding, g.original_length = gapless.encoder_delay, gapless.padding, gapless.original_length
        g.n_frames = len(lists_per)
        for k, a in (("lists_per_frame", a_lp), ("list_ptr", a_ptr), ("list_len", a_ll), ("scales_per_frame", a_sp),
                     ("scale_ptr", a_sptr), ("raw_ptr", a_rptr), ("raw_len", a_rl)):
            setattr(g, k, a.ctypes.data if a.size else None)
        out = C.c_void_p()
        check(lib.glc_frames_from_gather(C.byref(g), stream_id, C.byref(out)))
        return EncodedAudio(out.value)

    @staticmethod
    def from_records(sample_rate: int, n_samples: int, channels: int, records: np.ndarray) -> "EncodedAudio":
        """Assemble from the device path's fixed-size frame records (all shards, frame order)."""
        records = np.ascontiguousarray(records, np.uint8).reshape(-1)
        rec = lib.glc_record_bytes(channels)
        if rec == 0 or records.size % rec:
            raise GlcError(GLC_EINVAL, "record buffer is not a whole number of records")
        out = C.c_void_p()
        check(lib.glc_frames_from_records(sample_rate, n_samples, channels,
                                          records.ctypes.data_as(C.c_void_p), records.size // rec,
                                          C.byref(out)))
        return EncodedAudio(out.value)


    @staticmethod
    def from_compact(sample_rate: int, n_samples: int, channels: int, blobs) -> "EncodedAudio":
        """Assemble from compact blobs (one per shard, frame order): glc_frames_from_compact.
        Each blob is a bytes-like / uint8 array as produced by Encoder.compact_device_records or
        compact_records."""
        arrs = [np.ascontiguousarray(np.frombuffer(b, np.uint8) if isinstance(b, (bytes, bytearray, memoryview))
                                     else b, np.uint8).reshape(-1) for b in blobs]
        n = len(arrs)
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        sizes = (C.c_uint64 * max(n, 1))(*[a.size for a in arrs])
        out = C.c_void_p()
        check(lib.glc_frames_from_compact(sample_rate, n_samples, channels, ptrs, sizes, n, C.byref(out)))
        return EncodedAudio(out.value)


def _view_to_dict(v: GlcFramesView) -> dict:
    def take(ptr, n, t):
        if not n:
            return np.empty(0, t)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(t))), shape=(n,)).copy()
    d = {k: int(getattr(v, k)) for k in ("sample_rate", "channels", "total_samples", "encoder_delay", "padding",
                                         "original_length", "n_frames", "n_lists", "n_pairs", "n_scales", "n_raw")}
    nf = d["n_frames"]
    d["list_begin"] = take(v.list_begin, nf + 1, np.uint64)
    d["list_off"] = take(v.list_off, d["n_lists"] + 1, np.uint64)
    d["pairs"] = take(v.pairs, d["n_pairs"], np.uint32)
    d["scale_begin"] = take(v.scale_begin, nf + 1, np.uint64)
    d["scales"] = take(v.scales, d["n_scales"], np.float32)
    d["raw_tag"] = take(v.raw_tag, nf, np.uint8)
    d["raw_begin"] = take(v.raw_begin, nf + 1, np.uint64)
    d["raw"] = take(v.raw, d["n_raw"], np.int16)
    return d


def compact_bound(channels: int, n_frames: int) -> int:
    """Capacity a compact-blob buffer needs for n_frames frames (glc_compact_bound)."""
    return int(lib.glc_compact_bound(channels, n_frames))


def compact_store_bound(channels: int, lengths) -> int:
    """Arena bytes that hold the blobs of clips of `lengths` samples per channel whatever their content
    (glc_compact_store_bound: the sum of compact_bound over the clips)."""
    lens = _ints(lengths)
    arr = _c_array(C.c_uint64, lens)
    lay = GlcClipLayout(len(lens), channels, 0, 0, 0, 0, C.cast(arr, C.POINTER(C.c_uint64)))
    return int(lib.glc_compact_store_bound(C.byref(lay)))


def store_blobs(arena, entries) -> list:
    """The blobs Encoder.encode_compact_batch_tensor left in `arena`, as the list of arena slices that
    Decoder.decode_compact_batch_tensor takes: one download of `entries` (it waits for the encode), no copy of a
    blob.  None stands for a clip that did not fit (stored == 0)."""
    e = entries.cpu().tolist()
    return [arena[off:off + size] if (raw_stored >> 32) & 1 else None for off, size, _, raw_stored in e]


def store_crop_slots(length: int, channels: int):
    """(max_hops, max_frames): the hops and frames a crop of `length` samples per channel needs wherever it starts
    (glc_store_crop_slots) - the fixed slots a crop of Decoder.decode_store_crops_tensor owns."""
    if length < 0 or not 0 <= channels <= 0xFFFF:
        raise GlcError(GLC_EINVAL, "store_crop_slots: negative length or a channel count out of range")
    hops, frames = C.c_uint64(), C.c_uint64()
    check(lib.glc_store_crop_slots(length, channels, C.byref(hops), C.byref(frames)))
    return int(hops.value), int(frames.value)


def store_ragged_slots(length: int, channels: int):
    """(max_descs, max_frames): the hop descriptors and frames a ragged crop of `length` samples per channel needs
    whatever its start and valid length (glc_store_ragged_slots) - the fixed slots a crop of
    Decoder.decode_store_ragged_crops_tensor owns."""
    if length < 0 or not 0 <= channels <= 0xFFFF:
        raise GlcError(GLC_EINVAL, "store_ragged_slots: negative length or a channel count out of range")
    descs, frames = C.c_uint64(), C.c_uint64()
    check(lib.glc_store_ragged_slots(length, channels, C.byref(descs), C.byref(frames)))
    return int(descs.value), int(frames.value)


def compact_records(records: np.ndarray, channels: int) -> np.ndarray:
    """Host twin of the device compaction (glc_compact_records): records -> compact blob bytes."""
    records = np.ascontiguousarray(records, np.uint8).reshape(-1)
    rec = lib.glc_record_bytes(channels)
    if rec == 0 or records.size % rec:
        raise GlcError(GLC_EINVAL, "record buffer is not a whole number of records")
    nf = records.size // rec
    blob = np.empty(compact_bound(channels, nf), np.uint8)
    info = GlcCompactInfo()
    check(lib.glc_compact_records(records.ctypes.data_as(C.c_void_p), nf, channels, blob.ctypes.data_as(C.c_void_p),
                                  blob.size, C.byref(info)))
    return blob[:info.bytes].copy()


def frames_to_compact(encoded: "EncodedAudio") -> bytes:
    """The compact blob of a whole stream (glc_frames_to_compact): the inverse of EncodedAudio.from_compact, the
    bytes compact_records gives for the stream's records.  One upload puts it into a device store that
    Decoder.decode_compact_tensor / decode_compact_batch_tensor decode in place.  GlcError (GLC_EINVAL) for a
    stream a blob cannot hold (non-canonical lists, frames with another number of vectors than channels)."""
    info = GlcCompactInfo()
    rc = lib.glc_frames_to_compact(encoded._h, None, 0, C.byref(info))  # sizes the blob, or says why there is none
    if rc != GLC_EINVAL or info.bytes == 0:
        check(rc)
    blob = np.empty(info.bytes, np.uint8)
    check(lib.glc_frames_to_compact(encoded._h, blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(info)))
    return blob[:info.bytes].tobytes()


def compact_join(blobs, channels: Optional[int] = None) -> bytes:
    """The blob of a whole clip from its segment blobs in frame order (glc_compact_join): what a receiver of
    StreamEncoder.segments calls, and the host twin of join_segments_tensor - the header of the sums, then each of the
    five sections the segments' sections back to back.  channels: the clip's channel count; None takes it from the first
    blob's header (every segment must then agree with it, as with a given one).  GlcError (GLC_EINVAL) names the first
    unusable segment; an empty list is refused too."""
    arrs = [np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else np.ascontiguousarray(b, np.uint8).reshape(-1)
            for b in blobs]
    held = [np.concatenate([a, np.zeros(-a.size % 8, np.uint8)]).view(np.uint64) for a in arrs]  # 8-byte aligned copies
    ptrs = _c_array(C.c_void_p, [h.ctypes.data for h in held])
    sizes = _c_array(C.c_uint64, [a.size for a in arrs])
    if channels is None:
        channels = int(arrs[0][4:8].copy().view(np.uint32)[0]) if arrs and arrs[0].size >= 8 else 0
    if not 0 < channels <= 0xFFFF:
        raise GlcError(GLC_EINVAL, "compact_join: no channel count (an empty list, a blob without a header, or channels out of range)")
    info = GlcCompactInfo()
    rc = lib.glc_compact_join(ptrs, sizes, len(arrs), channels, None, 0, C.byref(info))  # sizes the blob, or says why there is none
    if rc != GLC_EINVAL or info.bytes == 0:
        check(rc)
    out = np.empty(info.bytes // 8 + 1, np.uint64)
    check(lib.glc_compact_join(ptrs, sizes, len(arrs), channels, out.ctypes.data_as(C.c_void_p), info.bytes, C.byref(info)))
    return out.view(np.uint8)[:info.bytes].tobytes()


def compact_cut(blob, first_frame: int, n_frames: int, channels: Optional[int] = None) -> bytes:
    """The blob of frames [first_frame, first_frame + n_frames) of a clip's blob (glc_compact_cut): the host twin of
    cut_clips_tensor and the inverse of compact_join - a fresh header, then the window's slice of each of the five
    sections.  channels: the clip's channel count; None takes it from the blob's header.  GlcError (GLC_EINVAL) says
    what is wrong with an unusable blob or window."""
    arr = np.frombuffer(bytes(blob), np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, np.uint8).reshape(-1)
    held = np.concatenate([arr, np.zeros(-arr.size % 8, np.uint8)]).view(np.uint64)  # an 8-byte aligned copy
    if channels is None:
        channels = int(arr[4:8].copy().view(np.uint32)[0]) if arr.size >= 8 else 0
    if not 0 < channels <= 0xFFFF:
        raise GlcError(GLC_EINVAL, "compact_cut: no channel count (a blob without a header, or channels out of range)")
    first_frame, n_frames = int(first_frame), int(n_frames)
    if first_frame < 0 or n_frames < 0:
        raise GlcError(GLC_EINVAL, "compact_cut: first_frame and n_frames must not be negative")
    info = GlcCompactInfo()
    src = held.ctypes.data_as(C.c_void_p)
    rc = lib.glc_compact_cut(src, arr.size, channels, first_frame, n_frames, None, 0, C.byref(info))  # sizes the piece, or says why there is none
    if rc != GLC_EINVAL or info.bytes == 0:
        check(rc)
    out = np.empty(info.bytes // 8 + 1, np.uint64)
    check(lib.glc_compact_cut(src, arr.size, channels, first_frame, n_frames, out.ctypes.data_as(C.c_void_p), info.bytes, C.byref(info)))
    return out.view(np.uint8)[:info.bytes].tobytes()


@dataclass
class CompactStatus:
    """glc_compact_status: what the device check of one compact blob found (include/glc.h GLC_COMPACT_*)."""
    flags: int
    n_bad_rows: int
    first_bad_row: int


def plan_encode(n_samples: int, channels: int) -> GlcPlan:
    """Frame count / padding of Encoder::encode (src/codec.rs:433-455); raises where it panics."""
    p = GlcPlan()
    check(lib.glc_plan_encode(n_samples, channels, C.byref(p)))
    return p


def plan_crop(n_samples: int, channels: int, start: int, length: int) -> GlcCropPlan:
    """The frames [first_frame, first_frame + n_frames) and hops [first_hop, first_hop + n_hops) that the crop
    [start, start + length) (samples per channel) of a clip of n_samples interleaved samples needs (glc_plan_crop);
    raises where it refuses: an empty crop, one that ends behind the clip, a clip the encoder refuses."""
    if start < 0 or length < 0:
        raise GlcError(GLC_EINVAL, "plan_crop: negative start or length")
    p = GlcCropPlan()
    check(lib.glc_plan_crop(n_samples, channels, C.byref(GlcCrop(start, length)), C.byref(p)))
    return p


_PCM_FORMATS = {np.dtype(np.int16): (GLC_PCM_S16, 16), np.dtype(np.int32): (GLC_PCM_S32, 32),
                np.dtype(np.float32): (GLC_PCM_F32, 32)}
_PCM_DTYPES = {GLC_PCM_S16: np.int16, GLC_PCM_S32: np.int32, GLC_PCM_F32: np.float32}


def _pcm_bits(fmt: int, width: int, bits: Optional[int], dtype) -> int:
    """The `bits` rule of every call that takes PCM: none for float32 samples (TypeError), 1..width for integer
    ones (GlcError), default the container's width."""
    if fmt == GLC_PCM_F32:
        if bits is not None:
            raise TypeError("bits applies to integer samples only")
        return 32
    bits = width if bits is None else int(bits)
    if not 1 <= bits <= width:
        raise GlcError(GLC_EINVAL, f"bits must be 1..{width} for {dtype} samples")
    return bits


def pcm_format(samples, bits: Optional[int] = None):
    """(flat C-contiguous array, glc_pcm_format, bits) of samples handed to an encoder: float32, or
    int16 / int32 holding `bits`-bit values (default: the container's width).  An array of any other
    dtype raises TypeError - nothing is cast silently; a plain sequence is taken as float32."""
    dt = getattr(samples, "dtype", None)
    if dt is None:
        samples, dt = np.asarray(samples, np.float32), np.dtype(np.float32)
    if np.dtype(dt) not in _PCM_FORMATS:
        raise TypeError(f"samples must be float32, int16 or int32, not {dt}")
    fmt, width = _PCM_FORMATS[np.dtype(dt)]
    return np.ascontiguousarray(samples).reshape(-1), fmt, _pcm_bits(fmt, width, bits, np.dtype(dt))


_TORCH_PCM_FORMATS = {}   # torch dtype -> (glc_pcm_format, container bits); filled by the first tensor call, torch is imported lazily


def _tensor_pcm_format(t, bits: Optional[int], what: str = "x"):
    """(glc_pcm_format, bits) of a torch tensor handed to a device batch call: float32, or int16 / int32 holding
    `bits`-bit values - the defaults and the checks pcm_format applies to integer arrays."""
    if not _TORCH_PCM_FORMATS:
        import torch
        _TORCH_PCM_FORMATS.update({getattr(torch, np.dtype(dt).name): f for dt, f in _PCM_FORMATS.items()})
    if getattr(t, "dtype", None) not in _TORCH_PCM_FORMATS:
        raise TypeError(f"{what} must be a float32, int16 or int32 CUDA tensor")
    fmt, width = _TORCH_PCM_FORMATS[t.dtype]
    return fmt, _pcm_bits(fmt, width, bits, t.dtype)


def _tensor_out_dtype(dtype, out):
    """torch.float32 or torch.int16 for the output of a device batch decode: an `out` tensor of int16 selects the
    format by itself; `dtype` (torch or numpy spelling) names it for a fresh output."""
    import torch
    if isinstance(out, torch.Tensor) and out.dtype == torch.int16:
        return torch.int16
    if dtype is None:
        return torch.float32
    name = str(dtype).replace("torch.", "") if isinstance(dtype, torch.dtype) else np.dtype(dtype).name
    if name not in ("float32", "int16"):
        raise TypeError(f"dtype must be float32 or int16, not {dtype}")
    return getattr(torch, name)


def _out_format(out) -> int:
    """glc_pcm_format of an output tensor that _tensor_out_dtype passed: int16 or float32."""
    return GLC_PCM_S16 if out.dtype.itemsize == 2 else GLC_PCM_F32


def _entry_in(name: str, fmt: int, bits: int):
    """Where the samples' format chooses the entry point: (`name`, ()) for float32 input, (`name`_int, (fmt, bits)) -
    the arguments that follow the samples - for integer PCM."""
    return (getattr(lib, name), ()) if fmt == GLC_PCM_F32 else (getattr(lib, name + "_int"), (fmt, bits))


def _entry_out(name: str, out):
    """Where the output's format chooses the entry point: `name` gives float32, `name`_i16 int16."""
    return getattr(lib, name + "_i16" if _out_format(out) == GLC_PCM_S16 else name)


def _ints(values) -> list:
    """A sequence or a tensor of integers as a list of int."""
    return [int(v) for v in (values.tolist() if hasattr(values, "tolist") else values)]


def _c_array(ctype, values):
    """A ctypes array of `values`, never of length 0: an empty batch still hands the C side a pointer."""
    return (ctype * max(len(values), 1))(*values)


def _clip_layout(t, planar: bool, what: str):
    """(GlcClipLayout, B, C, T) of a padded batch tensor (B, C, T) (planar) or (B, T, C): the strides between clips and
    planes are the tensor's own, so a slice of something bigger is described where it lies.  The samples of a plane,
    or the channels of an interleaved sample, are adjacent; an interleaved clip is dense.  Reads shape and strides
    only; that `t` is a CUDA tensor of the right dtype on the right device is _Ctx._tensor's rule."""
    if t.dim() != 3:
        raise TypeError(f"{what} must have shape (B, C, T) or (B, T, C)")
    if t.shape[2] > 1 and t.stride(2) != 1:
        raise TypeError(f"{what}: the innermost stride must be 1")
    if min(t.stride(0), t.stride(1)) < 0:
        raise TypeError(f"{what}: negative strides")
    b, c, n = (t.shape[0], t.shape[1], t.shape[2]) if planar else (t.shape[0], t.shape[2], t.shape[1])
    if not planar and b and c and n > 1 and t.stride(1) != c:
        raise TypeError(f"{what}: an interleaved clip must be dense (stride {c} between samples)")
    return GlcClipLayout(b, c, 1 if planar else 0, t.stride(0), t.stride(1) if planar else 0, n, None), b, c, n


def _set_lengths(lay: GlcClipLayout, lengths, b: int, t: int) -> list:
    """Give `lay` the true lengths of its clips: `b` integers in [0, t], a sequence or a tensor.  The array the
    layout points into is the layout's own attribute and lives as long as it; returns the lengths as a list."""
    lens = _ints(lengths)
    if len(lens) != b or any(v < 0 or v > t for v in lens):
        raise GlcError(GLC_EINVAL, f"lengths must hold {b} values in [0, {t}]")
    lay.lengths_array = _c_array(C.c_uint64, lens)
    lay.lengths = C.cast(lay.lengths_array, C.POINTER(C.c_uint64))
    return lens


class _on_torch_stream:
    """`with _on_torch_stream(ctx, device):` - the scope in which a context queues on torch's current stream of `device`,
    the one way the tensor methods reach the stream (any context class, a stub in a test).  Entered, it hands that stream to
    the context (set_stream); left, also by an exception, it restores the private stream (set_stream(0), which waits
    for what was queued).  The legacy default stream has no handle to hand over (0 means the private stream, which
    does not order itself against it): what torch has queued there - the fill of a fresh output, whatever produced
    the input - is waited for instead."""
    __slots__ = ("ctx", "device")

    def __init__(self, ctx: "_Ctx", device):
        self.ctx, self.device = ctx, device

    def __enter__(self):
        import torch
        s = torch.cuda.current_stream(self.device)
        if s.cuda_stream == 0:
            s.synchronize()
        self.ctx.set_stream(s.cuda_stream)

    def __exit__(self, *exc):
        self.ctx.set_stream(0)


class _Ctx:
    def __init__(self, sample_rate: int, device: int):
        h = C.c_void_p()
        check(lib.glc_ctx_create(device, sample_rate, C.byref(h)))
        self._h = h
        self.sample_rate = sample_rate
        self.device = device

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.glc_ctx_destroy(h)

    def close(self):
        self.__del__()

    def tables(self):
        """(cos_table[1024,2048], window[2048], norm, weights[1024], band_edges)."""
        T = np.empty((HOP_SIZE, FRAME_SIZE), np.float32)
        w = np.empty(FRAME_SIZE, np.float32)
        wt = np.empty(HOP_SIZE, np.float32)
        e = np.zeros(64, np.uint32)
        n = C.c_float()
        ne = C.c_uint32()
        check(lib.glc_ctx_tables(self._h, T.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p),
                                 C.byref(n), wt.ctypes.data_as(C.c_void_p),
                                 e.ctypes.data_as(C.c_void_p), C.byref(ne)), self._h)
        return T, w, np.float32(n.value), wt, e[:ne.value].copy()

    def set_stream(self, raw_stream: int) -> None:
        """Run this context's kernels on a caller-owned hipStream_t (0 restores the private stream).
        A handle is only meaningful inside the HIP runtime that created it: refused when the process
        has mapped two (libglc_hip.so loaded before torch, see _lib.py)."""
        if raw_stream:
            from ._lib import hip_runtimes_mapped
            rts = hip_runtimes_mapped()
            if len(rts) > 1:
                raise GlcError(GLC_EINVAL, f"two HIP runtimes are mapped ({rts}): a foreign hipStream_t must not cross; "
                                           "import torch before glc_amd")
        check(lib.glc_ctx_set_stream(self._h, C.c_void_p(raw_stream)), self._h)

    def synchronize(self) -> None:
        check(lib.glc_ctx_synchronize(self._h), self._h)

    def _tensor(self, t, what: str, dtypes, shape=None, contiguous: bool = True):
        """`t` as it is, or the refusal: `what` must be a (contiguous) CUDA tensor of one of `dtypes` (one torch dtype
        or a tuple) and, where `shape` is given, of its rank and sizes - None stands for any size - (TypeError), on
        this context's device (GlcError)."""
        import torch
        ok = isinstance(t, torch.Tensor) and t.is_cuda and (t.dtype in dtypes if isinstance(dtypes, tuple) else t.dtype == dtypes) \
            and (not contiguous or t.is_contiguous()) and (shape is None or t.dim() == len(shape))
        if ok and shape is not None:
            for want, got in zip(shape, t.shape):
                if want is not None and want != got:
                    ok = False
        if not ok:
            names = " or ".join(str(d).replace("torch.", "") for d in (dtypes if isinstance(dtypes, tuple) else (dtypes,)))
            of = "" if shape is None else f" of shape ({', '.join('n' if w is None else str(w) for w in shape)})"
            raise TypeError(f"{what} must be a {'contiguous ' if contiguous else ''}{names} CUDA tensor{of}")
        if t.get_device() != self.device:
            raise GlcError(GLC_EINVAL, f"{what} is on {t.device}, this context on device {self.device}")
        return t

    def _pcm_tensor(self, x, bits: Optional[int]):
        """(glc_pcm_format, bits) of the samples of a device batch call: `x` a 3-D CUDA tensor of a PCM dtype, any strides."""
        import torch
        return _tensor_pcm_format(self._tensor(x, "x", (torch.float32, torch.int16, torch.int32), (None, None, None), contiguous=False), bits)

    def _append_tensors(self, arena, cursor):
        """The arena and the cursor of the two calls that append to a store, checked."""
        import torch
        self._tensor(arena, "arena", torch.uint8, (None,))
        if self._tensor(cursor, "cursor", torch.int64, contiguous=False).numel() != 1:
            raise TypeError("cursor must be a one-element int64 CUDA tensor")

    def _out_tensor(self, out, shape, dtype, planar: bool, contiguous: bool = False):
        """(out, its GlcClipLayout, B, C, T) of a call that fills a padded batch: `out` None is a new zero-filled
        tensor of `shape` and `dtype` (what _tensor_out_dtype gave) on this context's device, a given one is held
        to _tensor and _clip_layout."""
        import torch
        if out is None:
            out = torch.zeros(shape, dtype=dtype, device=torch.device("cuda", self.device))
        self._tensor(out, "out", dtype, (None, None, None), contiguous)
        return (out,) + _clip_layout(out, planar, "out")

    def _compact_status(self, n: int) -> list:
        """One CompactStatus per blob of the last call that decoded `n` compact blobs on this context."""
        arr = (GlcCompactStatus * max(n, 1))()
        if n:
            check(lib.glc_decode_compact_last_status(self._h, arr, n), self._h)
        return [CompactStatus(int(a.flags), int(a.n_bad_rows), int(a.first_bad_row)) for a in arr[:n]]

    def compact_store_tensor(self, arena, entries, lengths, keep, out_arena=None, used_bytes=None):
        """Evict clips from a store and close the gaps (glc_store_compact_device).  arena: the 1-D uint8 CUDA tensor;
        entries: its (N, 4) int64 CUDA index; lengths: (N,) int64 CUDA, or None; keep: (N,) torch.bool / uint8 CUDA,
        non-zero = keep.  out_arena: None compacts in place, else a 1-D uint8 CUDA tensor that does not overlap
        `arena` receives the kept blobs.  used_bytes: a host bound on the bytes of `arena` in use (default: all of
        it); fewer rounds are queued in place, and an entry that reaches behind it is unusable.
        Returns (entries_out, lengths_out, new_index, n_out, cursor), all new CUDA tensors: (N, 4) int64 with the
        kept entries in front and zeros behind them, (N,) int64 or None, (N,) int64 - the new number of every old
        entry or -1 (dropped) / -2 (unusable) / -3 (out of order) -, and two one-element int64 tensors; `cursor` is
        what Encoder.encode_compact_batch_tensor takes to append.  Nothing is read on the host and nothing is copied
        to or from it; queued on torch's current stream.  The context's resident stream, decode session and
        last-info records are untouched."""
        import torch
        self._tensor(arena, "arena", torch.uint8, (None,))
        n = self._tensor(entries, "entries", torch.int64, (None, 4)).shape[0]
        if lengths is not None:
            self._tensor(lengths, "lengths", torch.int64, (n,))
        self._tensor(keep, "keep", (torch.bool, torch.uint8), (n,))
        if out_arena is not None:
            self._tensor(out_arena, "out_arena", torch.uint8, (None,))
        src_bytes = arena.numel()
        if used_bytes is not None:
            used_bytes = int(used_bytes)
            if not 0 <= used_bytes <= src_bytes:
                raise GlcError(GLC_EINVAL, f"used_bytes must lie in [0, {src_bytes}]")
            src_bytes = used_bytes
        dst, dst_bytes = (arena, src_bytes) if out_arena is None else (out_arena, out_arena.numel())
        dev = arena.device
        entries_out = torch.empty((n, 4), dtype=torch.int64, device=dev)
        lengths_out = torch.empty(n, dtype=torch.int64, device=dev) if lengths is not None else None
        new_index = torch.empty(n, dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        with _on_torch_stream(self, dev):
            check(lib.glc_store_compact_device(
                self._h, C.c_void_p(arena.data_ptr()), src_bytes, C.c_void_p(entries.data_ptr()),
                C.c_void_p(lengths.data_ptr()) if lengths is not None else None, n, C.c_void_p(keep.data_ptr()),
                C.c_void_p(dst.data_ptr()), dst_bytes, C.c_void_p(entries_out.data_ptr()),
                C.c_void_p(lengths_out.data_ptr()) if lengths is not None else None, C.c_void_p(new_index.data_ptr()),
                C.c_void_p(counts.data_ptr()), C.c_void_p(counts.data_ptr() + 8)), self._h)
        return entries_out, lengths_out, new_index, counts[0:1], counts[1:2]

    def join_segments_tensor(self, arena, entries, segs, out_arena, cursor, lengths=None, channels: Optional[int] = None):
        """Join the segments StreamEncoder.push_tensor stored into one blob per clip (glc_store_join_segments_device).
        arena: the 1-D uint8 CUDA tensor the segments lie in; entries: its (n_segs, 4) int64 CUDA index; segs: the host
        list [(stream, first_frame, n_frames)] in the same order, ascending by (stream, first_frame) - the segments of
        one stream value are one clip; out_arena / cursor: the destination store, as
        Encoder.encode_compact_batch_tensor takes them (the call appends at the cursor); lengths: per clip the samples
        per channel (host integers), or None; channels: the clips' channel count (default: this object's).
        Returns (entries_out, lengths_out, seg_status), new CUDA tensors: (n_clips, 4) int64 - all zero for a clip
        with an unusable segment -, (n_clips,) int64 or None, (n_segs,) int32 of GLC_COMPACT_* bits.  Nothing is read
        on the host and nothing but the table image is copied; queued on torch's current stream.  The context's
        resident stream, decode session and last-info records are untouched."""
        import torch
        channels = int(getattr(self, "channels", 0) if channels is None else channels)
        if not 0 < channels <= 0xFFFF:
            raise GlcError(GLC_EINVAL, "join_segments_tensor: channels must be 1..65535")
        segs = [tuple(int(v) for v in g) for g in segs]
        n = self._tensor(entries, "entries", torch.int64, (len(segs), 4)).shape[0]
        self._tensor(arena, "arena", torch.uint8, (None,))
        self._append_tensors(out_arena, cursor)
        n_clips = len({g[0] for g in segs})
        if lengths is not None:
            lengths = _ints(lengths)
            if len(lengths) != n_clips:
                raise GlcError(GLC_EINVAL, f"lengths must hold {n_clips} values, one per clip")
        dev = arena.device
        entries_out = torch.zeros((n_clips, 4), dtype=torch.int64, device=dev)
        lengths_out = torch.zeros(n_clips, dtype=torch.int64, device=dev) if lengths is not None else None
        seg_status = torch.zeros(n, dtype=torch.int32, device=dev)
        c_segs = _c_array(GlcStreamSeg, [GlcStreamSeg(*g) for g in segs])
        c_lens = _c_array(C.c_uint64, lengths) if lengths is not None else None
        with _on_torch_stream(self, dev):
            check(lib.glc_store_join_segments_device(
                self._h, C.c_void_p(arena.data_ptr()), arena.numel(), C.c_void_p(entries.data_ptr()), c_segs, n, c_lens,
                channels, C.c_void_p(out_arena.data_ptr()), out_arena.numel(), C.c_void_p(cursor.data_ptr()),
                C.c_void_p(entries_out.data_ptr()), C.c_void_p(lengths_out.data_ptr()) if lengths is not None else None,
                C.c_void_p(seg_status.data_ptr())), self._h)
        return entries_out, lengths_out, seg_status

    def cut_clips_tensor(self, arena, entries, cuts, out_arena, cursor, lengths=None, channels: Optional[int] = None):
        """Cut stored clips into frame ranges (glc_store_cut_device): split, trim, resend - the inverse of
        join_segments_tensor.  arena: the 1-D uint8 CUDA tensor the clips lie in; entries: its (N, 4) int64 CUDA index;
        cuts: an (n, 3) host integer array or a list of triples (clip, first_frame, n_frames), in any order, a clip any
        number of times, ranges may overlap; out_arena / cursor: the destination store, as
        Encoder.encode_compact_batch_tensor takes them (the call appends at the cursor); lengths: per piece the samples
        per channel (host integers, each planning to the piece's n_frames), or None for 1024 * n_frames; channels: the
        clips' channel count (default: this object's).
        Returns (entries_out, lengths_out, status), new CUDA tensors: (n, 4) int64 - all zero for a refused cut -,
        (n,) int64 - 0 for a refused cut -, (n,) int32 of GLC_COMPACT_* bits.  Nothing is read on the host and nothing
        but the table image is copied; queued on torch's current stream.  The context's resident stream, decode session
        and last-info records are untouched."""
        import torch
        channels = int(getattr(self, "channels", 0) if channels is None else channels)
        if not 0 < channels <= 0xFFFF:
            raise GlcError(GLC_EINVAL, "cut_clips_tensor: channels must be 1..65535")
        cuts = [tuple(int(v) for v in c) for c in (cuts.tolist() if isinstance(cuts, np.ndarray) else cuts)]
        if any(len(c) != 3 or min(c) < 0 for c in cuts):
            raise GlcError(GLC_EINVAL, "cut_clips_tensor: a cut is (clip, first_frame, n_frames), none of them negative")
        n = len(cuts)
        n_entries = self._tensor(entries, "entries", torch.int64, (None, 4)).shape[0]
        self._tensor(arena, "arena", torch.uint8, (None,))
        self._append_tensors(out_arena, cursor)
        if lengths is not None:
            lengths = _ints(lengths)
            if len(lengths) != n:
                raise GlcError(GLC_EINVAL, f"lengths must hold {n} values, one per cut")
        dev = arena.device
        entries_out = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        lengths_out = torch.zeros(n, dtype=torch.int64, device=dev)
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        c_cuts = _c_array(GlcStoreCut, [GlcStoreCut(*c) for c in cuts])
        c_lens = _c_array(C.c_uint64, lengths) if lengths is not None else None
        with _on_torch_stream(self, dev):
            check(lib.glc_store_cut_device(
                self._h, C.c_void_p(arena.data_ptr()), arena.numel(), C.c_void_p(entries.data_ptr()), n_entries, c_cuts, n, c_lens,
                channels, C.c_void_p(out_arena.data_ptr()), out_arena.numel(), C.c_void_p(cursor.data_ptr()),
                C.c_void_p(entries_out.data_ptr()), C.c_void_p(lengths_out.data_ptr()), C.c_void_p(status.data_ptr())), self._h)
        return entries_out, lengths_out, status

    def timer_begin(self) -> None:
        """Record a HIP event on the context's stream (device-side stopwatch)."""
        check(lib.glc_ctx_timer_begin(self._h), self._h)

    def timer_end(self) -> float:
        """Record a second event, wait for it, return elapsed milliseconds."""
        ms = C.c_float()
        check(lib.glc_ctx_timer_end(self._h, C.byref(ms)), self._h)
        return ms.value


class Encoder(_Ctx):
    """Encoder::new(sample_rate) — src/codec.rs:406."""

    def __init__(self, sample_rate: int, device: int = 0):
        super().__init__(sample_rate, device)

    def encode(self, samples, channels: int, bits: Optional[int] = None) -> EncodedAudio:
        """Encoder::encode(&mut self, samples: &[f32], channels: u16) — src/codec.rs:421.  int16 /
        int32 samples (of `bits` bits, default the container's width) are encoded as the reference
        encodes what its loaders make of them, s / 2^(bits-1) - widened on the device (glc_encode_int)."""
        pcm, fmt, bits = pcm_format(samples, bits)
        out = C.c_void_p()
        if fmt == GLC_PCM_F32:
            check(lib.glc_encode(self._h, pcm.ctypes.data_as(C.c_void_p), pcm.size, channels, C.byref(out)),
                  self._h)
        else:
            check(lib.glc_encode_int(self._h, pcm.ctypes.data_as(C.c_void_p), fmt, bits, pcm.size, channels,
                                     C.byref(out)), self._h)
        return EncodedAudio(out.value)

    def encode_batch(self, clips, channels: int, bits: Optional[int] = None) -> list:
        """glc_encode_batch: Encoder::encode of every clip of `clips` (a sequence of float32 arrays, each an
        independent stream of `channels` channels) in one call; the i-th EncodedAudio holds the bytes
        `encode(clips[i], channels)` gives.  Short clips share launch chains, uploads and downloads.
        A sequence of int16 or of int32 arrays (of `bits` bits, as in encode) goes through
        glc_encode_batch_int: the integers are uploaded and widened on the device.  One call has one sample
        format: a sequence that mixes dtypes raises GlcError(GLC_EINVAL) before any device work."""
        clips = list(clips)
        int_dt = {np.dtype(c.dtype) for c in clips if getattr(c, "dtype", None) in (np.int16, np.int32)}
        if not int_dt:
            if bits is not None:
                raise TypeError("bits applies to integer samples only")
            pcm, fmt = [np.ascontiguousarray(c, np.float32).reshape(-1) for c in clips], GLC_PCM_F32
        else:
            got = [pcm_format(c, bits) for c in clips]  # TypeError for a dtype that is no PCM format at all
            if len({f for _, f, _ in got}) != 1:
                raise GlcError(GLC_EINVAL, "encode_batch: the clips of one call have one dtype (int16, int32 or float32)")
            pcm, fmt, bits = [p for p, _, _ in got], got[0][1], got[0][2]
        n = len(pcm)
        ptrs = (C.c_void_p * max(n, 1))(*[p.ctypes.data for p in pcm])
        lens = (C.c_uint64 * max(n, 1))(*[p.size for p in pcm])
        outs = (C.c_void_p * max(n, 1))()
        if fmt == GLC_PCM_F32:
            check(lib.glc_encode_batch(self._h, ptrs, lens, n, channels, outs), self._h)
        else:
            check(lib.glc_encode_batch_int(self._h, ptrs, fmt, bits, lens, n, channels, outs), self._h)
        return [EncodedAudio(outs[i]) for i in range(n)]

    def widen_device(self, d_in: int, dtype, bits: int, n: int, d_out: int) -> None:
        """glc_pcm_widen_device: n int16 / int32 samples of `bits` bits at device address d_in ->
        float32 at d_out, s / 2^(bits-1).  Queued on the context's stream, not synchronised."""
        if np.dtype(dtype) not in _PCM_FORMATS:
            raise TypeError(f"samples must be float32, int16 or int32, not {np.dtype(dtype)}")
        check(lib.glc_pcm_widen_device(self._h, C.c_void_p(d_in), _PCM_FORMATS[np.dtype(dtype)][0], bits, n,
                                       C.c_void_p(d_out)), self._h)

    def encode_hooked(self, samples, channels: int, hook) -> EncodedAudio:
        """glc_encode_hooked: `hook(parts, frame_begin, frame_end)` is called each time a range of frames
        has arrived on the host (while the device works on later ones); `parts` is the dict of
        EncodedAudio.parts() for frames [0, frame_end).  A truthy return aborts the encode."""
        pcm = np.ascontiguousarray(samples, np.float32).reshape(-1)
        failure = []

        def tramp(_user, view, f0, f1):
            try:
                return 1 if hook(_view_to_dict(view.contents), int(f0), int(f1)) else 0
            except BaseException as e:  # no exception may cross the C frames
                failure.append(e)
                return 1
        cb = FRAMES_HOOK(tramp)
        out = C.c_void_p()
        rc = lib.glc_encode_hooked(self._h, pcm.ctypes.data_as(C.c_void_p), pcm.size, channels, cb, None, C.byref(out))
        if failure:
            raise failure[0]
        check(rc, self._h)
        return EncodedAudio(out.value)

    def encode_range_device(self, d_pcm: int, t0: int, t_count: int, n_samples: int, channels: int,
                            frame_begin: int, frame_end: int, d_records: int, d_coeffs: int = 0) -> None:
        """Device-resident frame range (body of the rayon loop, src/codec.rs:462-541).  Pointers
        are raw device addresses; work is queued on the context's stream, not synchronised."""
        check(lib.glc_encode_range_device(self._h, C.c_void_p(d_pcm), t0, t_count, n_samples, channels,
                                          frame_begin, frame_end, C.c_void_p(d_records),
                                          C.c_void_p(d_coeffs) if d_coeffs else None), self._h)

    def frames_from_device_records(self, d_records: int, n_frames: int, n_samples: int, channels: int) -> EncodedAudio:
        """EncodedAudio from records still on this context's device (device-side compaction)."""
        out = C.c_void_p()
        check(lib.glc_frames_from_device_records(self._h, C.c_void_p(d_records), n_frames, n_samples, channels,
                                                 C.byref(out)), self._h)
        return EncodedAudio(out.value)

    def compact_device_records(self, d_records: int, n_frames: int, channels: int, d_blob: int, cap: int) -> GlcCompactInfo:
        """Pack n_frames device records into the compact blob at device address d_blob
        (glc_compact_device_records); synchronises; returns the sizes (info.bytes travel)."""
        info = GlcCompactInfo()
        check(lib.glc_compact_device_records(self._h, C.c_void_p(d_records) if d_records else None, n_frames, channels,
                                             C.c_void_p(d_blob), cap, C.byref(info)), self._h)
        return info

    def encode_compact_tensor(self, x, channels: int):
        """Encode a contiguous float32 CUDA tensor of interleaved samples (1-D, or (frames, channels)) into its
        compact blob ON THE DEVICE: glc_encode_range_device + glc_compact_device_records into a uint8 CUDA tensor
        of glc_compact_bound bytes, returned sliced to info.bytes (its storage is 64-byte aligned, as the compact
        decode wants it) together with the GlcCompactInfo.  Runs on torch's current stream; synchronises (the
        sizes come back)."""
        import torch
        n = self._tensor(x, "x", torch.float32).numel()
        plan = plan_encode(n, channels)
        nf = plan.n_frames
        records = torch.empty(nf * int(lib.glc_record_bytes(channels)), dtype=torch.uint8, device=x.device)
        blob = torch.empty(compact_bound(channels, nf), dtype=torch.uint8, device=x.device)
        with _on_torch_stream(self, x.device):
            self.encode_range_device(x.data_ptr(), 0, plan.per_channel, n, channels, 0, nf, records.data_ptr())
            info = self.compact_device_records(records.data_ptr(), nf, channels, blob.data_ptr(), blob.numel())
        return blob[:info.bytes], info

    def encode_compact_batch_tensor(self, x, lengths=None, planar: bool = True, arena=None, cursor=None, bits: Optional[int] = None):
        """Encode every clip of a padded batch into its own compact blob, the blobs back to back in an arena the
        DEVICE allocates from (glc_encode_batch_device_compact).  `x`: a float32 CUDA tensor (B, C, T) (planar) or
        (B, T, C), innermost stride 1, any slice of something bigger; lengths: per clip its true samples per channel
        (default T) - what lies behind them is not read.  arena: a 1-D uint8 CUDA tensor whose first byte is 64-byte
        aligned (None: a new one of compact_store_bound bytes); cursor: a one-element int64 CUDA tensor holding the
        first free byte of the arena (None: a new zero).  Passing the same arena and cursor again appends.
        Returns (arena, cursor, entries): entries an (B, 4) int64 CUDA tensor, one glc_store_entry per clip as
        {offset, bytes, n_pairs, n_raw_rows | stored << 32}; blob i is arena[offset : offset + bytes] when stored
        (store_blobs cuts them).  A clip that does not fit is not stored, and the cursor counts on: its final value
        is the arena size that would have sufficed.  Queued on torch's current stream as RoundTrip.apply_batch_tensor
        queues; nothing is copied to the host and the C call does not synchronise (restoring the context's private
        stream afterwards waits for the queued work, as in every *_tensor method).
        An int16 / int32 tensor holds `bits`-bit integer PCM (default: the container's width; the checks of
        Encoder.encode): glc_encode_batch_device_compact_int widens it in the gather, and the blobs are those of the
        widened clips, byte for byte."""
        import torch
        fmt, bits = self._pcm_tensor(x, bits)
        lay, b, ch, n = _clip_layout(x, planar, "x")
        if not 0 < ch <= 0xFFFF:
            raise GlcError(GLC_EINVAL, f"x: {ch} channels")
        if lengths is not None:
            _set_lengths(lay, lengths, b, n)
        if arena is None:
            arena = torch.empty(max(int(lib.glc_compact_store_bound(C.byref(lay))), 64), dtype=torch.uint8, device=x.device)
        if cursor is None:
            cursor = torch.zeros(1, dtype=torch.int64, device=x.device)
        self._append_tensors(arena, cursor)
        entries = torch.zeros((b, 4), dtype=torch.int64, device=x.device)
        call, ints = _entry_in("glc_encode_batch_device_compact", fmt, bits)
        with _on_torch_stream(self, x.device):
            check(call(
                self._h, C.c_void_p(x.data_ptr()), *ints, C.byref(lay), C.c_void_p(arena.data_ptr()), arena.numel(),
                C.c_void_p(cursor.data_ptr()), C.c_void_p(entries.data_ptr())), self._h)
        return arena, cursor, entries

    def mdct_forward_device(self, d_pcm: int, t0: int, t_count: int, n_samples: int, channels: int,
                            frame_begin: int, frame_end: int, d_coeffs: int) -> None:
        """Window + mdct_block only (src/codec.rs:476-485) for a frame range, device-resident."""
        check(lib.glc_mdct_forward_device(self._h, C.c_void_p(d_pcm), t0, t_count, n_samples, channels,
                                          frame_begin, frame_end, C.c_void_p(d_coeffs)), self._h)


class Decoder(_Ctx):
    """Decoder::new(channels, sample_rate) — src/codec.rs:581.  `channels` is accepted and
    ignored exactly like the reference (quirk Q4): the stream's header decides."""

    def __init__(self, channels: int, sample_rate: int, device: int = 0):
        super().__init__(sample_rate, device)
        self.channels = channels

    @staticmethod
    def _progress(sender, kind: str, value) -> None:
        """Progress (src/codec.rs:71-79) delivered to an optional callable(kind, value) in place of
        the crossbeam Sender: kinds 'Status', 'Decoding', 'Complete' as sent at :609, :713, :736."""
        if sender is not None:
            sender(kind, value)

    @staticmethod
    def _out_dtype(dtype) -> np.dtype:
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.int16)):
            raise TypeError(f"decoded samples are float32 or int16, not {dt}")
        return dt

    def decode(self, encoded: EncodedAudio, progress_sender=None, out: Optional[np.ndarray] = None,
               dtype=np.float32) -> np.ndarray:
        """Decoder::decode — src/codec.rs:744-768 (overlap-add, gapless trim).  `out` (optional, not
        in the reference): an array of `dtype` of at least total_samples to decode into, for callers
        that reuse a buffer - pages that were touched before take the D2H copies much faster.
        dtype=np.int16: the samples as the reference's 16-bit writers narrow them,
        (s * 32767).clamp(-32768, 32767) as i16, narrowed on the device (glc_decode_i16)."""
        dt = self._out_dtype(dtype)
        if progress_sender is not None:  # the reference decodes through decode_streaming (:747)
            chunks = [c.samples for c in self.decode_streaming(encoded, progress_sender, dtype=dt)]
            allv = np.concatenate(chunks) if chunks else np.empty(0, dt)
            g = encoded.gapless_info
            if allv.size > g.encoder_delay:
                allv = allv[g.encoder_delay:]
            return allv[:g.original_length].copy()
        n = lib.glc_decoded_len(encoded._h)
        if out is None:
            out = np.empty(n, dt)
        elif out.dtype != dt or not out.flags.c_contiguous or out.size < n:
            raise GlcError(GLC_EINVAL, f"out must be a C-contiguous {dt} array of at least total_samples")
        got = C.c_uint64()
        fn = lib.glc_decode if dt == np.float32 else lib.glc_decode_i16
        check(fn(self._h, encoded._h, out.ctypes.data_as(C.c_void_p), n, C.byref(got)), self._h)
        return out[:got.value]

    def decode_batch(self, encoded_list, out: Optional[np.ndarray] = None, dtype=np.float32) -> list:
        """glc_decode_batch: Decoder::decode of every stream of `encoded_list` (all of one channel count)
        in one call.  Returns one array of `dtype` per stream, views into ONE packed array - `out` when
        given (C-contiguous, of `dtype`, at least the sum of the streams' total_samples), as in decode.
        dtype=np.int16: narrowed on the device as in decode (glc_decode_batch_i16)."""
        dt = self._out_dtype(dtype)
        encs = list(encoded_list)
        n = len(encs)
        handles = (C.c_void_p * max(n, 1))(*[e._h for e in encs])
        offsets = (C.c_uint64 * (n + 1))()
        total = sum(int(lib.glc_decoded_len(e._h)) for e in encs)
        if out is None:
            out = np.empty(total, dt)
        elif out.dtype != dt or not out.flags.c_contiguous or out.size < total:
            raise GlcError(GLC_EINVAL, f"out must be a C-contiguous {dt} array of at least the streams' total_samples")
        fn = lib.glc_decode_batch if dt == np.float32 else lib.glc_decode_batch_i16
        check(fn(self._h, handles, n, out.ctypes.data_as(C.c_void_p), out.size, offsets), self._h)
        return [out[offsets[i]:offsets[i + 1]] for i in range(n)]

    def resident_stream(self) -> int:
        """Identity of the stream whose sparse rows this context holds on the device (0: none)."""
        return int(lib.glc_ctx_resident_stream(self._h))

    def decode_resident(self, stream_id: int, out: np.ndarray) -> np.ndarray:
        """glc_decode_resident: Decoder::decode of the resident stream without an EncodedAudio."""
        got = C.c_uint64()
        check(lib.glc_decode_resident(self._h, stream_id, out.ctypes.data_as(C.c_void_p), out.size, C.byref(got)), self._h)
        return out[:got.value]

    def decode_device(self, encoded: EncodedAudio, d_all: int, cap_all: int):
        """Device-resident decode of the whole un-trimmed stream into device memory at address
        d_all; returns (start, n): the window Decoder::decode would return (src/codec.rs:756-765).
        Queued on the context's stream, not synchronised."""
        start = C.c_uint64()
        n = C.c_uint64()
        check(lib.glc_decode_device(self._h, encoded._h, C.c_void_p(d_all), cap_all, C.byref(start), C.byref(n)),
              self._h)
        return start.value, n.value

    def decode_range_device(self, encoded: EncodedAudio, hop_begin: int, hop_end: int, d_out: int, cap: int) -> None:
        """One shard of the decode: hops [hop_begin, hop_end) of the un-trimmed stream into device
        memory at address d_out (glc_decode_range_device).  Queued, not synchronised."""
        check(lib.glc_decode_range_device(self._h, encoded._h, hop_begin, hop_end, C.c_void_p(d_out), cap), self._h)

    def decode_range_device_i16(self, encoded: EncodedAudio, hop_begin: int, hop_end: int, d_out: int, cap: int) -> None:
        """decode_range_device writing int16 samples, narrowed as Decoder.decode(dtype=np.int16) does
        (glc_decode_range_device_i16).  Queued, not synchronised."""
        check(lib.glc_decode_range_device_i16(self._h, encoded._h, hop_begin, hop_end, C.c_void_p(d_out), cap), self._h)

    def decode_device_records(self, d_records: int, n_frames: int, n_samples: int, channels: int, d_out: int, cap: int) -> int:
        """glc_decode_device_records: Decoder::decode of the stream that n_frames frame records at device
        address d_records describe (as Encoder.encode_range_device left them) into device memory at d_out,
        gapless-trimmed; returns the number of samples.  The decoder's row tables are built on the device:
        nothing crosses to the host.  Queued on the context's stream, not synchronised."""
        n = C.c_uint64()
        check(lib.glc_decode_device_records(self._h, C.c_void_p(d_records), n_frames, n_samples, channels,
                                            C.c_void_p(d_out), cap, C.byref(n)), self._h)
        return n.value

    def decode_device_compact(self, d_blob: int, blob_bytes: int, n_samples: int, channels: int, d_out: int, cap: int) -> int:
        """glc_decode_device_compact on raw device addresses; returns the number of samples written.  Queued on the
        context's stream, not synchronised."""
        n = C.c_uint64()
        check(lib.glc_decode_device_compact(self._h, C.c_void_p(d_blob), blob_bytes, n_samples, channels, C.c_void_p(d_out),
                                            cap, C.byref(n)), self._h)
        self._compact_clips = 1
        return n.value

    def decode_compact_tensor(self, blob, n_samples: int, out=None):
        """Decode ONE compact blob where it lies in device memory (glc_decode_device_compact): `blob` a 1-D uint8
        CUDA tensor whose first byte is 64-byte aligned, n_samples the stream's interleaved length, the channel
        count the decoder was made with.  Returns the n_samples decoded samples as a float32 CUDA tensor (`out`,
        when given: 1-D contiguous float32, at least n_samples long; its first n_samples elements are returned).
        Queued on torch's current stream as RoundTrip.apply_tensor queues; nothing touches the host."""
        import torch
        self._tensor(blob, "blob", torch.uint8, (None,))
        if out is None:
            out = torch.empty(n_samples, dtype=torch.float32, device=blob.device)
        self._tensor(out, "out", torch.float32, (None,))
        with _on_torch_stream(self, blob.device):
            n = self.decode_device_compact(blob.data_ptr(), blob.numel(), n_samples, self.channels, out.data_ptr(), out.numel())
        return out[:n]

    def _batch_out(self, blobs, lens, planar: bool, out, dtype=None):
        """The checked blobs of a decode_compact_* batch call, their addresses and sizes as the C call takes them, the
        output tensor (None: a new zero-filled one of T = max(lens)) and its glc_clip_layout with `lens` set."""
        import torch
        b, ch = len(blobs), self.channels
        for i, t in enumerate(blobs):
            self._tensor(t, f"blobs[{i}]", torch.uint8, (None,))
        t_max = max(lens, default=0)
        out, lay, ob, oc, ot = self._out_tensor(out, (b, ch, t_max) if planar else (b, t_max, ch), _tensor_out_dtype(dtype, out), planar)
        if ob != b or oc != ch:
            raise GlcError(GLC_EINVAL, f"out has shape {tuple(out.shape)} for {b} clips of {ch} channels")
        _set_lengths(lay, lens, b, ot)
        return _c_array(C.c_void_p, [t.data_ptr() for t in blobs]), _c_array(C.c_uint64, [t.numel() for t in blobs]), out, lay

    def decode_compact_batch_tensor(self, blobs, n_samples, lengths=None, planar: bool = True, out=None, dtype=None):
        """Decode one compact blob per clip into ONE padded batch tensor (glc_decode_batch_device_compact).  blobs: B
        1-D uint8 CUDA tensors (64-byte aligned, anywhere in device memory); n_samples: per clip its interleaved
        length; lengths: per clip its samples per channel (default n_samples[i] // channels).  out: a float32 CUDA
        tensor (B, C, T) (planar) or (B, T, C) with innermost stride 1 - a slice of something bigger works - or
        None: a new zero-filled one with T = max(lengths).  The first lengths[i] samples of clip i are what
        decode_compact_tensor gives for that blob; no other element is written.  One launch chain per round
        whatever B.  Queued on torch's current stream; returns the output.
        dtype=torch.int16 (or an int16 `out`, which selects the format by itself): 16-bit PCM narrowed on the device as
        decode(dtype=np.int16) narrows (glc_decode_batch_device_compact_i16)."""
        b = len(blobs)
        ns = _ints(n_samples)
        lens = [v // self.channels for v in ns] if lengths is None else _ints(lengths)
        if len(ns) != b or len(lens) != b:
            raise GlcError(GLC_EINVAL, f"n_samples and lengths must hold {b} values")
        ptrs, sizes, out, lay = self._batch_out(blobs, lens, planar, out, dtype)
        with _on_torch_stream(self, out.device):
            check(_entry_out("glc_decode_batch_device_compact", out)(
                self._h, ptrs, sizes, _c_array(C.c_uint64, ns), C.c_void_p(out.data_ptr()), C.byref(lay)), self._h)
        self._compact_clips = b
        return out

    def decode_compact_crops_tensor(self, blobs, n_samples, starts, lengths, planar: bool = True, out=None, dtype=None):
        """Decode a WINDOW of each of B stored clips into one padded batch tensor (glc_decode_crops_device_compact):
        entry i is samples [starts[i], starts[i] + lengths[i]) per channel of what decode_compact_tensor gives for
        blobs[i] (n_samples[i] its interleaved length), bit for bit; only the frames a window needs are decoded.
        lengths: per crop, or one int for all.  The same blob may appear any number of times.  out: as in
        decode_compact_batch_tensor ((B, C, L) planar / (B, L, C), a slice of something bigger works), or None: a
        new zero-filled one with L = max(lengths).  No element outside the crops is written.  One launch chain per
        round whatever B.  Queued on torch's current stream; returns the output.  last_compact_status() afterwards:
        one status per crop, bad rows counted inside the window (in the stream's row numbering).
        dtype=torch.int16 (or an int16 `out`): the crops as 16-bit PCM (glc_decode_crops_device_compact_i16)."""
        b = len(blobs)
        ns, st = _ints(n_samples), _ints(starts)
        lens = [int(lengths)] * b if isinstance(lengths, (int, np.integer)) else _ints(lengths)
        if len(ns) != b or len(st) != b or len(lens) != b:
            raise GlcError(GLC_EINVAL, f"n_samples, starts and lengths must hold {b} values")
        if any(v < 0 for v in st):
            raise GlcError(GLC_EINVAL, "starts must not be negative")
        ptrs, sizes, out, lay = self._batch_out(blobs, lens, planar, out, dtype)
        crops = _c_array(GlcCrop, [GlcCrop(a, n) for a, n in zip(st, lens)])
        with _on_torch_stream(self, out.device):
            check(_entry_out("glc_decode_crops_device_compact", out)(
                self._h, ptrs, sizes, _c_array(C.c_uint64, ns), crops, C.c_void_p(out.data_ptr()), C.byref(lay)), self._h)
        self._compact_clips = b
        return out

    def decode_store_crops_tensor(self, arena, entries, lengths, clips, starts, length: int, max_length: int,
                                  planar: bool = True, out=None, dtype=None):
        """Draw B crops of `length` samples per channel from the store as Encoder.encode_compact_batch_tensor left it
        (glc_decode_crops_device_store): crop i is samples [starts[i], starts[i] + length) of stored clip clips[i].
        arena: the uint8 CUDA tensor; entries: the (N, 4) int64 CUDA tensor the encode returned, or torch.cat of
        several; lengths: (N,) int64 CUDA, samples per channel of every stored clip; clips, starts: (B,) int64 CUDA
        (torch.randint on the device, or anything else); max_length: a host upper bound of lengths.  None of the
        tensors is read on the host and nothing is uploaded: the work of this method does not depend on B.  out: a
        float32 CUDA tensor (B, C, length) (planar) or (B, length, C) with innermost stride 1 - a slice of something
        bigger works - or None: a new zero-filled one.  Every usable crop is bit for bit decode_compact_crops_tensor's;
        a crop whose entry (flag 64) or selection (flag 128) is unusable is +0.0.  No element outside the crops is
        written.  Queued on torch's current stream; returns the output.  last_compact_status() afterwards: one
        status per crop.  dtype=torch.int16 (or an int16 `out`): the crops as 16-bit PCM, an unusable one 0
        (glc_decode_crops_device_store_i16)."""
        b, length, max_length, out, lay = self._store_draw_tensors(arena, entries, lengths, clips, starts, length, max_length, planar, out, dtype)
        with _on_torch_stream(self, out.device):
            check(_entry_out("glc_decode_crops_device_store", out)(
                self._h, C.c_void_p(arena.data_ptr()), arena.numel(), C.c_void_p(entries.data_ptr()),
                C.c_void_p(lengths.data_ptr()), entries.shape[0], max_length, C.c_void_p(clips.data_ptr()),
                C.c_void_p(starts.data_ptr()), length, C.c_void_p(out.data_ptr()), C.byref(lay)), self._h)
        self._compact_clips = b
        return out

    def _store_draw_tensors(self, arena, entries, lengths, clips, starts, length, max_length, planar: bool, out, dtype):
        """The checked tensors of a draw from the store -> (B, length, max_length, out, its GlcClipLayout); `out` None
        is a new zero-filled tensor of B crops of `length` samples."""
        import torch
        ch = self.channels
        dtype = _tensor_out_dtype(dtype, out)
        self._tensor(arena, "arena", torch.uint8, (None,))
        self._tensor(entries, "entries", torch.int64, (None, 4))
        for t, name in ((lengths, "lengths"), (clips, "clips"), (starts, "starts")):
            self._tensor(t, name, torch.int64, (None,))
        if lengths.shape[0] != entries.shape[0] or starts.shape[0] != clips.shape[0]:
            raise GlcError(GLC_EINVAL, "one length per entry and one start per clip index")
        b, length, max_length = clips.shape[0], int(length), int(max_length)
        if length < 0 or max_length < 0:
            raise GlcError(GLC_EINVAL, "length and max_length must not be negative")
        out, lay, ob, oc, ot = self._out_tensor(out, (b, ch, length) if planar else (b, length, ch), dtype, planar)
        if ob != b or oc != ch or ot != length:
            raise GlcError(GLC_EINVAL, f"out has shape {tuple(out.shape)} for {b} crops of {ch} channels and {length} samples")
        return b, length, max_length, out, lay

    def decode_store_ragged_crops_tensor(self, arena, entries, lengths, clips, starts, length: int, max_length: int, want=None,
                                         planar: bool = True, out=None, dtype=None, valid=None):
        """decode_store_crops_tensor for a ragged corpus (glc_decode_ragged_crops_device_store): every crop owns a row of
        `length` samples per channel, takes v = min(want[i], lengths[clips[i]] - starts[i]) of them from its clip -
        bit for bit decode_compact_crops_tensor's crop {starts[i], v} - and the rest of the row is +0.0; valid[i] = v.
        A selection is usable when 0 <= starts[i] < the clip's length and 1 <= want[i] <= length: clips shorter than
        `length`, starts near a clip's end and max_length < length are all fine.  want: (B,) int64 CUDA, or None: every
        crop wants `length`.  valid: (B,) int64 CUDA, or None: a new one.  The other arguments, the flags of an
        unusable crop (which is +0.0, valid 0) and last_compact_status() are decode_store_crops_tensor's; nothing is
        read on the host and nothing is uploaded.  Queued on torch's current stream; returns (out, valid).
        dtype=torch.int16 (or an int16 `out`): 16-bit PCM, padding and unusable crops 0
        (glc_decode_ragged_crops_device_store_i16)."""
        import torch
        b, length, max_length, out, lay = self._store_draw_tensors(arena, entries, lengths, clips, starts, length, max_length, planar, out, dtype)
        if want is not None:
            self._tensor(want, "want", torch.int64, (b,))
        if valid is None:
            valid = torch.zeros(b, dtype=torch.int64, device=out.device)
        self._tensor(valid, "valid", torch.int64, (b,))
        with _on_torch_stream(self, out.device):
            check(_entry_out("glc_decode_ragged_crops_device_store", out)(
                self._h, C.c_void_p(arena.data_ptr()), arena.numel(), C.c_void_p(entries.data_ptr()),
                C.c_void_p(lengths.data_ptr()), entries.shape[0], max_length, C.c_void_p(clips.data_ptr()),
                C.c_void_p(starts.data_ptr()), C.c_void_p(want.data_ptr()) if want is not None else None, length,
                C.c_void_p(out.data_ptr()), C.byref(lay), C.c_void_p(valid.data_ptr())), self._h)
        self._compact_clips = b
        return out, valid

    def last_compact_status(self):
        """glc_decode_compact_last_status: per blob of the last decode_compact_* call a CompactStatus (flags 0 and
        no bad rows for a blob that passed every check).  Synchronises."""
        return self._compact_status(getattr(self, "_compact_clips", 0))

    def imdct_device(self, encoded: EncodedAudio, frame_begin: int, frame_end: int, d_blocks: int) -> None:
        """Dequant + imdct_block + window (src/codec.rs:651-675) alone for a frame range:
        d_blocks[(frame - frame_begin) * ch + c][2048] on the device (glc_imdct_device)."""
        check(lib.glc_imdct_device(self._h, encoded._h, frame_begin, frame_end, C.c_void_p(d_blocks)), self._h)

    def decode_streaming(self, encoded: EncodedAudio, progress_sender=None, dtype=np.float32) -> Iterator[AudioChunk]:
        """Decoder::decode_streaming — src/codec.rs:595-741: yields AudioChunk until is_last
        (dtype=np.int16: chunks of narrowed samples, glc_decode_stream_next_i16)."""
        import time as _time
        dt = self._out_dtype(dtype)
        nxt = lib.glc_decode_stream_next if dt == np.float32 else lib.glc_decode_stream_next_i16
        t0 = _time.perf_counter()
        total_frames = encoded.info().n_frames
        self._progress(progress_sender, "Status", f"Starting streaming decode of {total_frames} frames")
        check(lib.glc_decode_stream_begin(self._h, encoded._h), self._h)
        ch = encoded.header.channels
        cap = FRAMES_PER_CHUNK * HOP_SIZE * ch  # the last chunk is < 500 frames + the tail hop
        done = 0
        while True:
            buf = np.empty(cap, dt)
            n = C.c_uint64()
            last = C.c_int()
            check(nxt(self._h, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(last)), self._h)
            done += FRAMES_PER_CHUNK
            if not last.value and total_frames:
                self._progress(progress_sender, "Decoding", min(done, total_frames) / total_frames * 100.0)
            yield AudioChunk(buf[:n.value].copy(), bool(last.value))
            if last.value:
                self._progress(progress_sender, "Complete",
                               f"Decoded {total_frames} frames in {_time.perf_counter() - t0:.2f}s")
                return


@dataclass
class RoundTripInfo:
    """What a round trip encoded: the counts EncodedAudio.info() gives for Encoder.encode of the same samples,
    and len(EncodedAudio.to_bytes()) of it."""
    n_frames: int
    n_raw_frames: int
    total_nnz: int
    serialized_bytes: int


class RoundTrip(_Ctx):
    """Encoder::encode followed by Decoder::decode as one call (glc_roundtrip, glc_roundtrip_device): what the
    codec does to audio - the reference's own "encode, decode, compare" tests, or a degradation stage in
    front of a model.  The samples are those of Decoder.decode(Encoder.encode(x)), bit for bit; no stream is
    assembled on the host, the decoder reads the encoder's frame records where they are on the device."""

    def __init__(self, sample_rate: int, device: int = 0):
        super().__init__(sample_rate, device)

    def apply(self, samples, channels: int, bits: Optional[int] = None, dtype=np.float32,
              out: Optional[np.ndarray] = None) -> np.ndarray:
        """Decoder.decode(Encoder.encode(samples, channels, bits), dtype=dtype) of a numpy array (float32, or
        int16 / int32 of `bits` bits as in Encoder.encode): one upload, one download.  `out`: as in
        Decoder.decode."""
        dt = Decoder._out_dtype(dtype)
        pcm, fmt, bits = pcm_format(samples, bits)
        if out is None:
            out = np.empty(pcm.size, dt)
        elif out.dtype != dt or not out.flags.c_contiguous or out.size < pcm.size:
            raise GlcError(GLC_EINVAL, f"out must be a C-contiguous {dt} array of at least as many samples as the input")
        got = C.c_uint64()
        check(lib.glc_roundtrip(self._h, pcm.ctypes.data_as(C.c_void_p), fmt, bits, pcm.size, channels,
                                out.ctypes.data_as(C.c_void_p), GLC_PCM_F32 if dt == np.float32 else GLC_PCM_S16,
                                out.size, C.byref(got)), self._h)
        return out[:got.value]

    def apply_device(self, d_pcm: int, n_samples: int, channels: int, d_out: int, cap: int) -> int:
        """glc_roundtrip_device on raw device addresses (interleaved float32 in, float32 out); returns the
        number of samples written.  Queued on the context's stream, not synchronised."""
        n = C.c_uint64()
        check(lib.glc_roundtrip_device(self._h, C.c_void_p(d_pcm), n_samples, channels, C.c_void_p(d_out), cap,
                                       C.byref(n)), self._h)
        return n.value

    def apply_tensor(self, x, channels: int):
        """The round trip of a contiguous float32 CUDA torch.Tensor - interleaved 1-D, or of shape (frames,
        channels) - into a new tensor of the same shape on the same device.  The work is queued on torch's
        current stream (set_stream) behind whatever fills `x` there, and the result is ready for torch ops on
        that stream: no torch.cuda.synchronize() is needed on either side.  The context's private stream is
        restored before the call returns, which waits for the queued work (glc_ctx_set_stream).  Raises
        GlcError where set_stream does (two HIP runtimes mapped)."""
        import torch
        self._tensor(x, "x", torch.float32)
        if x.dim() == 2:
            if x.shape[1] != channels:
                raise GlcError(GLC_EINVAL, f"a 2-D tensor is (frames, channels): got {tuple(x.shape)} for {channels} channels")
        elif x.dim() != 1:
            raise GlcError(GLC_EINVAL, "the tensor is interleaved 1-D or of shape (frames, channels)")
        out = torch.empty_like(x)
        with _on_torch_stream(self, x.device):
            n = self.apply_device(x.data_ptr(), x.numel(), channels, out.data_ptr(), out.numel())
        assert n == x.numel()
        return out

    def apply_batch_tensor(self, x, lengths=None, planar: bool = True, out=None, out_planar: Optional[bool] = None,
                           bits: Optional[int] = None, out_dtype=None):
        """The round trip of every clip of a padded batch in one call (glc_roundtrip_batch_device).  `x`: a float32
        CUDA tensor of shape (B, C, T) (planar) or (B, T, C), innermost stride 1; the other strides are taken from
        the tensor, so a slice of something bigger works without a copy.  lengths: per clip its true number of
        samples per channel (B integers, a sequence or a tensor; default: T for all).  In the output the first
        lengths[i] samples of clip i are Decoder.decode(Encoder.encode(them)), bit for bit what apply_tensor gives
        for that clip alone; no other element of it is written.
        out: None - a new tensor like x, zero-filled, so the padding behind short clips is zero; x itself - in
        place; or a float32 CUDA tensor of its own, whose layout is out_planar (default: as `planar`) and which
        must not overlap x.  Queued on torch's current stream as apply_tensor queues; returns the output.
        An int16 / int32 `x` holds `bits`-bit integer PCM (default: the container's width), widened on the device as
        Encoder.encode widens it; out_dtype (torch.float32, the default, or torch.int16; an int16 `out` selects it by
        itself) is the output's format, int16 narrowed as Decoder.decode(dtype=np.int16) narrows
        (glc_roundtrip_batch_device_pcm).  In place needs the same format on both sides."""
        import torch
        out_planar = planar if out_planar is None else bool(out_planar)
        fmt, bits = self._pcm_tensor(x, bits)
        out_dtype = _tensor_out_dtype(out_dtype, out)
        lin, b, ch, n = _clip_layout(x, planar, "x")
        if not 0 < ch <= 0xFFFF:
            raise GlcError(GLC_EINVAL, f"x: {ch} channels")
        if lengths is not None:
            _set_lengths(lin, lengths, b, n)
        if out is None:   # like x: its strides where it is dense, and no shape to build
            out = torch.zeros_like(x, dtype=out_dtype) if planar == out_planar else \
                torch.zeros_like(x.transpose(1, 2), dtype=out_dtype, memory_format=torch.contiguous_format)
        want = tuple(x.shape) if planar == out_planar else (x.shape[0], x.shape[2], x.shape[1])
        out, lout = self._out_tensor(out, want, out_dtype, out_planar)[:2]
        if tuple(out.shape) != want:
            raise GlcError(GLC_EINVAL, f"out has shape {tuple(out.shape)}, expected {want}")
        lout.lengths, lout.lengths_array = lin.lengths, getattr(lin, "lengths_array", None)   # one array, held by both
        with _on_torch_stream(self, x.device):
            if fmt == GLC_PCM_F32 and _out_format(out) == GLC_PCM_F32:
                check(lib.glc_roundtrip_batch_device(self._h, C.c_void_p(x.data_ptr()), C.byref(lin), C.c_void_p(out.data_ptr()),
                                                     C.byref(lout)), self._h)
            else:   # the one entry point that takes both formats as arguments
                check(lib.glc_roundtrip_batch_device_pcm(self._h, C.c_void_p(x.data_ptr()), fmt, bits, C.byref(lin),
                                                         C.c_void_p(out.data_ptr()), _out_format(out), C.byref(lout)), self._h)
        self._batch_clips = b
        return out

    def apply_batch_device(self, d_pcm: int, layout_in: "GlcClipLayout", d_out: int, layout_out: "GlcClipLayout") -> None:
        """glc_roundtrip_batch_device on raw device addresses and glc_clip_layout structures (_lib.GlcClipLayout).
        Queued on the context's stream, not synchronised."""
        check(lib.glc_roundtrip_batch_device(self._h, C.c_void_p(d_pcm), C.byref(layout_in), C.c_void_p(d_out),
                                             C.byref(layout_out)), self._h)
        self._batch_clips = int(layout_in.n_clips)

    def last_batch_info(self):
        """glc_roundtrip_batch_last_info: per clip of the last apply_batch_* call the RoundTripInfo that last_info()
        gives after a round trip of that clip alone (synchronises)."""
        n = getattr(self, "_batch_clips", 0)
        arr = (GlcRoundtripInfo * max(n, 1))()
        check(lib.glc_roundtrip_batch_last_info(self._h, arr, n), self._h)
        return [RoundTripInfo(i.n_frames, i.n_raw_frames, i.total_nnz, i.serialized_bytes) for i in arr[:n]]

    def resident_stream(self) -> int:
        """0 after every apply* call: a round trip leaves no stream resident on its context."""
        return int(lib.glc_ctx_resident_stream(self._h))

    def last_info(self) -> RoundTripInfo:
        """glc_roundtrip_last_info: counts and serialized size of the stream the last apply* call encoded
        (synchronises)."""
        i = GlcRoundtripInfo()
        check(lib.glc_roundtrip_last_info(self._h, C.byref(i)), self._h)
        return RoundTripInfo(i.n_frames, i.n_raw_frames, i.total_nnz, i.serialized_bytes)


def plan_stream_push(received: int, n_new: int, finish: bool = False) -> GlcStreamPushPlan:
    """What a push of n_new samples per channel completes on a lane of a streaming encode that has `received` so
    far (glc_plan_stream_push): first_frame, n_frames and the samples held back afterwards; raises where a finish
    ends a stream the encoder refuses (<= 512 samples per channel)."""
    if received < 0 or n_new < 0:
        raise GlcError(GLC_EINVAL, "plan_stream_push: negative count")
    p = GlcStreamPushPlan()
    check(lib.glc_plan_stream_push(received, n_new, 1 if finish else 0, C.byref(p)))
    return p


class StreamEncoder(_Ctx):
    """Encoder::encode fed in chunks: n_streams independent lanes of `channels` channels on one context
    (glc_stream_enc_*).  A lane pushed in any chunking serialises to the bytes Encoder.encode gives for the
    concatenation.  Use .push / .segments / .encoded (host samples) or .push_tensor (device samples), not both."""

    def __init__(self, sample_rate: int, channels: int, n_streams: int = 1, device: int = 0):
        super().__init__(sample_rate, device)
        self.channels, self.n_streams = int(channels), int(n_streams)
        self._s = None
        if not 0 < self.channels <= 0xFFFF or self.n_streams <= 0:
            raise GlcError(GLC_EINVAL, "StreamEncoder: channels must be 1..65535 and n_streams positive")
        s = C.c_void_p()
        check(lib.glc_stream_enc_open(self._h, self.channels, self.n_streams, C.byref(s)), self._h)
        self._s = s

    def __del__(self):
        s, self._s = getattr(self, "_s", None), None
        if s:
            lib.glc_stream_enc_close(s)  # before its context
        super().__del__()

    @property
    def max_push(self) -> int:
        """Samples per channel one lane may take in one device push."""
        return int(lib.glc_stream_enc_max_push(self.channels))

    def _finish_flags(self, finish):
        if finish is None:
            return None, None
        flags = np.ascontiguousarray(np.asarray(finish).astype(bool).astype(np.uint8).reshape(-1))
        if flags.size != self.n_streams:
            raise GlcError(GLC_EINVAL, f"finish must hold {self.n_streams} flags")
        return flags, flags.ctypes.data_as(C.c_void_p)

    def push(self, chunks, finish=None, bits: Optional[int] = None) -> None:
        """chunks: per lane the interleaved samples it receives (None or empty: nothing), all float32 or all int16 /
        int32 of `bits` bits; finish: per lane whether this chunk ends its stream (None: no lane).  Synchronises."""
        if self.n_streams == 1 and (chunks is None or hasattr(chunks, "dtype")):
            chunks = [chunks]
        if len(chunks) != self.n_streams:
            raise GlcError(GLC_EINVAL, f"chunks must hold {self.n_streams} arrays")
        if self.n_streams == 1 and isinstance(finish, (bool, int)):
            finish = [finish]
        arrs, fmt = [], None
        for c in chunks:
            if c is None or len(c) == 0:
                arrs.append(None)
                continue
            a, f, b = pcm_format(c, bits)
            if fmt is not None and (f, b) != fmt:
                raise TypeError("the chunks of one push must share one sample format")
            fmt = (f, b)
            arrs.append(a)
        fmt = fmt or (GLC_PCM_F32, 32)
        ptrs = (C.c_void_p * self.n_streams)(*[a.ctypes.data if a is not None else None for a in arrs])
        ns = (C.c_uint64 * self.n_streams)(*[a.size if a is not None else 0 for a in arrs])
        flags, fp = self._finish_flags(finish)
        check(lib.glc_stream_enc_push(self._s, ptrs, fmt[0], fmt[1], ns, fp), self._h)

    def segments(self, i: int = 0) -> list:
        """[(first_frame, n_frames, blob bytes)] of lane i: the segments host pushes have completed and .encoded has
        not taken - what a sender ships; glc_frames_from_compact assembles them."""
        n = C.c_uint64()
        check(lib.glc_stream_enc_segments(self._s, i, C.byref(n)), self._h)
        out = []
        for k in range(n.value):
            p, nb, f0, nf = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64()
            check(lib.glc_stream_enc_segment(self._s, i, k, C.byref(p), C.byref(nb), C.byref(f0), C.byref(nf)), self._h)
            out.append((f0.value, nf.value, C.string_at(p.value, nb.value)))
        return out

    def encoded(self, i: int = 0) -> EncodedAudio:
        """The finished stream of lane i as EncodedAudio; the lane is fresh afterwards."""
        out = C.c_void_p()
        check(lib.glc_stream_enc_frames(self._s, i, C.byref(out)), self._h)
        return EncodedAudio(out.value)

    def reset(self, i: int = 0) -> None:
        """Lane i back to "nothing received"."""
        check(lib.glc_stream_enc_reset(self._s, i), self._h)

    def push_tensor(self, x, lengths, finish, arena, cursor, planar: bool = True, bits: Optional[int] = None):
        """glc_stream_enc_push_device on torch's current stream.  x: a float32 / int16 / int32 CUDA tensor (B, C, T)
        (planar) or (B, T, C) with B == n_streams, innermost stride 1; lengths: per lane the samples per channel it
        receives (None: T); finish: per lane flags or None; arena / cursor as Encoder.encode_compact_batch_tensor takes
        them.  Returns (entries, segs): an (n_segs, 4) int64 CUDA tensor of glc_store_entry words and the host list
        [(lane, first_frame, n_frames)] in the same order.  Nothing is copied to the host."""
        import torch
        fmt, bits = self._pcm_tensor(x, bits)
        lay, b, ch, n = _clip_layout(x, planar, "x")
        if b != self.n_streams or ch != self.channels:
            raise GlcError(GLC_EINVAL, f"x must hold {self.n_streams} lanes of {self.channels} channels")
        _set_lengths(lay, [n] * b if lengths is None else lengths, b, n)
        self._append_tensors(arena, cursor)
        flags, fp = self._finish_flags(finish)
        entries = torch.zeros((b, 4), dtype=torch.int64, device=x.device)
        segs = (GlcStreamSeg * b)()
        n_segs = C.c_uint64()
        with _on_torch_stream(self, x.device):
            check(lib.glc_stream_enc_push_device(self._s, C.c_void_p(x.data_ptr()), fmt, bits, C.byref(lay), fp,
                                                 C.c_void_p(arena.data_ptr()), arena.numel(), C.c_void_p(cursor.data_ptr()),
                                                 C.c_void_p(entries.data_ptr()), segs, C.byref(n_segs)), self._h)
        return entries[:n_segs.value], [(g.stream, g.first_frame, g.n_frames) for g in segs[:n_segs.value]]


def plan_stream_dec_push(frames_done: int, n_frames: int, finish: bool = False, total_len: int = 0) -> GlcStreamDecPlan:
    """What a push of n_frames frames emits on a lane of a streaming decode that has taken frames_done so far
    (glc_plan_stream_dec_push): first_sample and n_samples, per channel; raises where a finish's total_len does not
    plan to exactly frames_done + n_frames frames."""
    if frames_done < 0 or n_frames < 0 or total_len < 0:
        raise GlcError(GLC_EINVAL, "plan_stream_dec_push: negative count")
    p = GlcStreamDecPlan()
    check(lib.glc_plan_stream_dec_push(frames_done, n_frames, 1 if finish else 0, total_len, C.byref(p)))
    return p


class StreamDecoder(_Ctx):
    """Decoder::decode fed in segments: n_streams independent lanes of `channels` channels on one context
    (glc_stream_dec_*).  The concatenation of a lane's outputs over any chunking is bit for bit Decoder.decode of the
    stream its segments assemble to.  Use .push (host blobs) or .push_tensor (a device arena), not both."""

    def __init__(self, sample_rate: int, channels: int, n_streams: int = 1, device: int = 0):
        super().__init__(sample_rate, device)
        self.channels, self.n_streams = int(channels), int(n_streams)
        self._s = None
        self._n_segs = 0
        if not 0 < self.channels <= 0xFFFF or self.n_streams <= 0:
            raise GlcError(GLC_EINVAL, "StreamDecoder: channels must be 1..65535 and n_streams positive")
        s = C.c_void_p()
        check(lib.glc_stream_dec_open(self._h, self.channels, self.n_streams, C.byref(s)), self._h)
        self._s = s

    def __del__(self):
        s, self._s = getattr(self, "_s", None), None
        if s:
            lib.glc_stream_dec_close(s)  # before its context
        super().__del__()

    @property
    def max_push(self) -> int:
        """Frames one lane may take in one push."""
        return int(lib.glc_stream_dec_max_push(self.channels))

    def frames_done(self, i: int = 0) -> int:
        n = C.c_uint64()
        check(lib.glc_stream_dec_frames_done(self._s, i, C.byref(n)), self._h)
        return n.value

    def reset(self, i: int = 0) -> None:
        """Lane i back to "no frame taken"."""
        check(lib.glc_stream_dec_reset(self._s, i), self._h)

    def _lane_args(self, finish, total_len):
        b = self.n_streams
        if b == 1 and isinstance(finish, (bool, int)):
            finish = [finish]
        if b == 1 and isinstance(total_len, int):
            total_len = [total_len]
        fin = [False] * b if finish is None else [bool(v) for v in finish]
        tot = [0] * b if total_len is None else [int(v) for v in total_len]
        if len(fin) != b or len(tot) != b:
            raise GlcError(GLC_EINVAL, f"finish and total_len must hold {b} values")
        return fin, tot

    def _plans(self, frames, fin, tot):
        return [plan_stream_dec_push(self.frames_done(i), frames[i], fin[i], tot[i]) if frames[i] or fin[i] else None
                for i in range(self.n_streams)]

    def push(self, segments_per_lane, finish=None, total_len=None, dtype=np.float32) -> list:
        """segments_per_lane: per lane a list of (first_frame, n_frames, blob bytes) - what StreamEncoder.segments
        gives - in frame order (None or empty: nothing); finish / total_len: per lane whether this push ends its stream
        and the stream's samples per channel.  Returns per lane the interleaved samples the push emits (float32, or
        int16 narrowed as Decoder.decode(dtype=np.int16) narrows).  Synchronises."""
        b, ch = self.n_streams, self.channels
        if b == 1 and (segments_per_lane is None or (len(segments_per_lane) and isinstance(segments_per_lane[0], tuple))):
            segments_per_lane = [segments_per_lane]
        if len(segments_per_lane) != b:
            raise GlcError(GLC_EINVAL, f"segments_per_lane must hold {b} lists")
        dt = Decoder._out_dtype(dtype)
        fin, tot = self._lane_args(finish, total_len)
        flat = [(i, f0, nf, bytes(blob)) for i, lane in enumerate(segments_per_lane) for (f0, nf, blob) in (lane or [])]
        frames = [sum(nf for (_, nf, _) in (lane or [])) for lane in segments_per_lane]
        plans = self._plans(frames, fin, tot)
        outs = [np.empty((p.n_samples if p else 0) * ch, dtype=dt) for p in plans]
        n = len(flat)
        keep = [np.frombuffer(bytearray(blob) + bytearray(8), dtype=np.uint8) for (_, _, _, blob) in flat]
        ptrs = (C.c_void_p * max(n, 1))(*[k.ctypes.data for k in keep])
        nbytes = (C.c_uint64 * max(n, 1))(*[len(blob) for (_, _, _, blob) in flat])
        segs = (GlcStreamSeg * max(n, 1))(*[GlcStreamSeg(i, f0, nf) for (i, f0, nf, _) in flat])
        flags = (C.c_uint8 * b)(*[1 if v else 0 for v in fin])
        totals = (C.c_uint64 * b)(*tot)
        optrs = (C.c_void_p * b)(*[o.ctypes.data if o.size else None for o in outs])
        n_out = (C.c_uint64 * b)()
        check(lib.glc_stream_dec_push(self._s, ptrs, nbytes, segs, n, C.cast(flags, C.c_void_p), totals, optrs,
                                      GLC_PCM_S16 if dt == np.int16 else GLC_PCM_F32, n_out), self._h)
        self._n_segs = n
        return outs

    def push_tensor(self, arena, entries, segs, finish=None, total_len=None, planar: bool = True, out=None, dtype=None):
        """glc_stream_dec_push_device on torch's current stream.  arena: the contiguous 1-D uint8 CUDA tensor the
        segments lie in; entries: the (n_segs, 4) int64 CUDA tensor of glc_store_entry words and segs: the host list
        [(lane, first_frame, n_frames)] StreamEncoder.push_tensor returned (concatenated over pushes, ascending by lane
        and frame).  Returns (out, lengths): a (B, C, T) (planar) or (B, T, C) CUDA tensor, float32 or int16 (`dtype`
        or `out`'s), T the longest span of the push - `out` is filled when given, a fresh tensor is zero outside the
        spans - and per lane the samples per channel the push emitted.  Nothing is copied to the host."""
        import torch
        b, ch = self.n_streams, self.channels
        self._tensor(arena, "arena", torch.uint8, (None,))
        segs = [(int(a), int(f0), int(nf)) for (a, f0, nf) in segs]
        n = len(segs)
        if n:
            self._tensor(entries, "entries", torch.int64, (n, 4))
        fin, tot = self._lane_args(finish, total_len)
        frames = [0] * b
        for (a, _, nf) in segs:
            if not 0 <= a < b:
                raise GlcError(GLC_EINVAL, "segs: no such lane")
            frames[a] += nf
        lens = [p.n_samples if p else 0 for p in self._plans(frames, fin, tot)]
        t = max(max(lens), 1)
        shape = (b, ch, t) if planar else (b, t, ch)
        out, lay, ob, oc, ot = self._out_tensor(out, shape, _tensor_out_dtype(dtype, out), planar, contiguous=True)
        if ob != b or oc != ch or ot < max(lens):
            raise TypeError(f"out must be a contiguous CUDA tensor of shape {shape} or longer in time")
        _set_lengths(lay, lens, b, ot)
        lay.length = 0   # a push has no common length: every lane's span is in `lengths`
        c_segs = _c_array(GlcStreamSeg, [GlcStreamSeg(a, f0, nf) for (a, f0, nf) in segs])
        flags = (C.c_uint8 * b)(*[1 if v else 0 for v in fin])
        totals = (C.c_uint64 * b)(*tot)
        with _on_torch_stream(self, arena.device):
            check(lib.glc_stream_dec_push_device(self._s, C.c_void_p(arena.data_ptr()), arena.numel(),
                                                 C.c_void_p(entries.data_ptr()) if n else None, c_segs, n,
                                                 C.cast(flags, C.c_void_p), totals, C.c_void_p(out.data_ptr()),
                                                 _out_format(out), C.byref(lay)), self._h)
        self._n_segs = n
        return out, lens

    def last_compact_status(self):
        """glc_decode_compact_last_status: one CompactStatus per SEGMENT of the last push.  Synchronises."""
        return self._compact_status(self._n_segs)


def save_encoded(encoded: EncodedAudio, path) -> None:
    """src/codec.rs:774-779"""
    check(lib.glc_save(encoded._h, str(path).encode()))


def load_encoded(path) -> EncodedAudio:
    """src/codec.rs:781-786"""
    out = C.c_void_p()
    check(lib.glc_load(str(path).encode(), C.byref(out)))
    return EncodedAudio(out.value)


def load_wav(path):
    """audio::load_wav (src/audio.rs:39-64) -> (samples f32 interleaved, sample_rate, channels)."""
    ptr = C.c_void_p()
    n = C.c_uint64()
    sr = C.c_uint32()
    ch = C.c_uint16()
    check(lib.glc_wav_load(str(path).encode(), C.byref(ptr), C.byref(n), C.byref(sr), C.byref(ch)))
    try:
        out = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(n.value,)).copy() \
            if n.value else np.empty(0, np.float32)
    finally:
        lib.glc_free(ptr)
    return out, sr.value, ch.value


def _f32_or_i16(samples):
    """Samples for a 16-bit writer: an int16 array is written as it is, anything else as float32."""
    if getattr(samples, "dtype", None) == np.int16:
        return np.ascontiguousarray(samples).reshape(-1), True
    return np.ascontiguousarray(samples, np.float32).reshape(-1), False


def export_to_wav(path, samples, sample_rate: int, channels: int) -> None:
    """audio::export_to_wav (src/audio.rs:100-132): 16-bit PCM (int16 samples: already narrowed)."""
    s, narrowed = _f32_or_i16(samples)
    fn = lib.glc_wav_save16_i16 if narrowed else lib.glc_wav_save16
    check(fn(str(path).encode(), s.ctypes.data_as(C.c_void_p), s.size, sample_rate, channels))


def _take_f32(ptr, n):
    try:
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(n,)).copy() if n \
            else np.empty(0, np.float32)
    finally:
        lib.glc_free(ptr)


def encode_flac_with_level(samples, sample_rate: int, channels: int, compression_level: int) -> bytes:
    """flac::encode_flac_with_level (src/flac.rs:947-1053): the reference's own FLAC encoder
    (int16 samples: already narrowed)."""
    s, narrowed = _f32_or_i16(samples)
    if not 0 <= int(compression_level) <= 255 or not 0 <= int(channels) <= 0xFFFF:
        raise GlcError(-1, "compression_level is a u8 and channels a u16 in the reference")
    ptr = C.c_void_p()
    n = C.c_uint64()
    fn = lib.glc_flac_encode_i16 if narrowed else lib.glc_flac_encode
    check(fn(s.ctypes.data_as(C.c_void_p), s.size, sample_rate, channels, compression_level, C.byref(ptr), C.byref(n)))
    try:
        return C.string_at(ptr, n.value)
    finally:
        lib.glc_free(ptr)


def encode_flac(samples, sample_rate: int, channels: int) -> bytes:
    """flac::encode_flac (src/flac.rs:1056-1063): compression level 5."""
    return encode_flac_with_level(samples, sample_rate, channels, 5)


def export_to_flac_with_level(path, samples, sample_rate: int, channels: int, compression_level: int) -> None:
    """flac::export_to_flac_with_level (src/flac.rs:1066-1077)."""
    s, narrowed = _f32_or_i16(samples)
    fn = lib.glc_flac_save_i16 if narrowed else lib.glc_flac_save
    check(fn(str(path).encode(), s.ctypes.data_as(C.c_void_p), s.size, sample_rate, channels, compression_level))


def export_to_flac(path, samples, sample_rate: int, channels: int) -> None:
    """audio::export_to_flac (src/audio.rs:87-96) = flac::export_to_flac (src/flac.rs:1080-1087)."""
    export_to_flac_with_level(path, samples, sample_rate, channels, 5)


def load_flac(path):
    """audio::load_flac (src/audio.rs:68-85) -> (samples f32 interleaved, sample_rate, channels)."""
    ptr = C.c_void_p()
    n = C.c_uint64()
    sr = C.c_uint32()
    ch = C.c_uint16()
    check(lib.glc_flac_load(str(path).encode(), C.byref(ptr), C.byref(n), C.byref(sr), C.byref(ch)))
    return _take_f32(ptr, n.value), sr.value, ch.value


def decode_flac(data: bytes):
    """In-memory form of load_flac."""
    ptr = C.c_void_p()
    n = C.c_uint64()
    sr = C.c_uint32()
    ch = C.c_uint16()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data) if data else (C.c_uint8 * 1)()
    check(lib.glc_flac_decode(C.cast(buf, C.c_void_p), len(data), C.byref(ptr), C.byref(n), C.byref(sr), C.byref(ch)))
    return _take_f32(ptr, n.value), sr.value, ch.value


def load_audio_file_lossless(path):
    """audio::load_audio_file_lossless (src/audio.rs:19-36): dispatch on the lower-cased extension."""
    import os
    ext = os.path.splitext(str(path))[1]
    if not ext:
        raise GlcError(-1, "No file extension")
    ext = ext[1:].lower()
    if ext == "wav":
        return load_wav(path)
    if ext == "flac":
        return load_flac(path)
    raise GlcError(-1, f"Unsupported file format: {ext}")


def load_audio_file_pcm(path):
    """load_audio_file_lossless before the widening (glc_audio_load_pcm) -> (samples, bits,
    sample_rate, channels): int16 for integer sources of at most 16 bits, int32 for wider ones,
    float32 for float WAV - what Encoder.encode(samples, channels, bits=bits) takes."""
    ptr = C.c_void_p()
    fmt = C.c_int()
    bits = C.c_uint32()
    n = C.c_uint64()
    sr = C.c_uint32()
    ch = C.c_uint16()
    check(lib.glc_audio_load_pcm(str(path).encode(), C.byref(ptr), C.byref(fmt), C.byref(bits), C.byref(n),
                                 C.byref(sr), C.byref(ch)))
    try:
        dt = np.dtype(_PCM_DTYPES[fmt.value])
        out = np.frombuffer(C.string_at(ptr, n.value * dt.itemsize), dt).copy() if n.value else np.empty(0, dt)
    finally:
        lib.glc_free(ptr)
    return out, bits.value, sr.value, ch.value
