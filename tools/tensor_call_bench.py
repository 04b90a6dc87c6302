"""Host cost of a call of the nine batch, store and stream torch-tensor methods: a small batch, where the Python in
front of the C entry point is the larger share of a call.

    python tools/tensor_call_bench.py [--root CHECKOUT] [--reps 300] [--warmup 20] [--stream default|side]

Every timed call ends with ctx.synchronize(); the figure of a method is the median over --reps calls in microseconds, one
JSON line in all.  --root names the checkout whose package is measured (default: the one this file lies in), so two
trees are compared by running the one tool on both, alternating.  --stream side makes a torch.cuda.Stream current, so
that the calls hand over a real handle instead of waiting for torch's legacy default stream."""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--stream", choices=("default", "side"), default="default")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch

    import glc_amd as g

    sr, ch, b, t = 48000, 2, 4, 2048 + 600                      # four clips of three frames
    rng = np.random.RandomState(3)
    tt = np.arange(t) / sr
    x = torch.from_numpy(np.stack([[0.3 * np.sin(2 * np.pi * rng.uniform(100, 4000) * tt + c) for c in range(ch)]
                                   for _ in range(b)]).astype(np.float32)).cuda()
    if a.stream == "side":
        torch.cuda.set_stream(torch.cuda.Stream())
    enc, dec, rt = g.Encoder(sr), g.Decoder(ch, sr), g.RoundTrip(sr)
    se, sd = g.StreamEncoder(sr, ch, n_streams=b), g.StreamDecoder(sr, ch, n_streams=b)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")
    arena, cursor, entries = enc.encode_compact_batch_tensor(x)
    used = int(cursor.item())
    blobs, ns = g.store_blobs(arena, entries), [t * ch] * b
    lengths_t, keep = i64([t] * b), torch.ones(b, dtype=torch.uint8, device="cuda")
    clips_t, starts_t = i64(list(range(b))), i64([7 * i for i in range(b)])
    out, crop_out, rt_out = torch.zeros_like(x), torch.zeros(b, ch, 1000, device="cuda"), torch.zeros_like(x)
    seg_arena, seg_cursor = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda"), i64([0])
    other = torch.zeros_like(arena)

    def stream_enc():
        seg_cursor.zero_()
        return se.push_tensor(x, None, [True] * b, seg_arena, seg_cursor)
    seg_entries, segs = stream_enc()
    seg_entries = seg_entries.clone()

    def encode_batch():
        cursor.zero_()
        enc.encode_compact_batch_tensor(x, arena=arena, cursor=cursor)
    calls = [
        ("compact_store_tensor", enc, lambda: enc.compact_store_tensor(arena, entries, lengths_t, keep, out_arena=other, used_bytes=used)),
        ("encode_compact_batch_tensor", enc, encode_batch),
        ("decode_compact_batch_tensor", dec, lambda: dec.decode_compact_batch_tensor(blobs, ns, out=out)),
        ("decode_compact_batch_tensor, fresh out", dec, lambda: dec.decode_compact_batch_tensor(blobs, ns)),
        ("decode_compact_crops_tensor", dec, lambda: dec.decode_compact_crops_tensor(blobs, ns, [0] * b, 1000, out=crop_out)),
        ("decode_store_crops_tensor", dec, lambda: dec.decode_store_crops_tensor(arena, entries, lengths_t, clips_t, starts_t, 1000, t, out=crop_out)),
        ("apply_batch_tensor", rt, lambda: rt.apply_batch_tensor(x, out=rt_out)),
        ("apply_batch_tensor, fresh out", rt, lambda: rt.apply_batch_tensor(x)),
        ("StreamEncoder.push_tensor", se, stream_enc),
        ("StreamDecoder.push_tensor", sd, lambda: sd.push_tensor(seg_arena, seg_entries, segs, finish=[True] * b, total_len=[t] * b, out=out)),
    ]
    result = {"root": os.path.abspath(a.root), "stream": a.stream, "reps": a.reps, "clips": b, "channels": ch, "samples_per_channel": t, "median_us": {}}
    for name, ctx, call in calls:
        for _ in range(a.warmup):
            call()
        ctx.synchronize()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            times.append(time.perf_counter() - t0)
        result["median_us"][name] = round(statistics.median(times) * 1e6, 2)
    print(json.dumps(result))
    for c in (enc, dec, rt, se, sd):
        c.close()


if __name__ == "__main__":
    main()
