#!/usr/bin/env python3
"""bench.py — Msamples/s of the device-resident encode hot path on MI355X.

Workload (BASELINE.json configs[1]): batch-encode 4096 frames x 1024 samples of 48 kHz stereo
synthetic PCM per GPU.  A "step" is one pass of the hot path (K1 windowed MDCT, K2 scale /
thresholds / quantiser / raw decision) over that batch, from interleaved f32 PCM resident in HBM to
fixed-size frame records resident in HBM.  With N > 1 ranks the stream is N x 4096 frames long and
rank r encodes the contiguous frame range [4096 r, 4096 (r+1)) from its own PCM shard + halo (weak
scaling, no data-path collective inside a step); the job then ends with the north_star's single
gather: every rank compacts its records on its device and the compact blobs go to rank 0.  For
N > 1 that gather is INSIDE the timed region (`value` = all samples / (K steps + one gather));
the gather-free figure is reported beside it.

Contract: `python bench.py --gpus N --steps K --warmup W` prints ONE JSON line.  With N > 1 and no
WORLD_SIZE in the environment this process starts the N ranks itself (before touching the GPU) and
relays rank 0's line; under `torch.distributed.run` it is one of the ranks.

A plain run does only what the headline needs: set-up, spin-up and warm-up, the K timed steps (and
for N > 1 the gather), the result line.  `--full` adds every measurement reported beside the
headline (K1 kernel leg and rooflines, the kernel K1 replaced, other sample rates, the record sanity
check, host boundary, decode, CPU baseline, the N > 1 assembly check).  `--dump-outputs DIR` writes
rank 0's records of the last timed step as float32 .npy files (see `record_arrays`).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SR, CH = 48000, 2
FRAMES_PER_GPU = 4096
HOP = 1024
FLOP_PER_SAMPLE = 4096.0          # 2048 mul + 2048 add per channel-sample
BYTES_PER_SAMPLE = 4.0 + 2.0 + 6.0 / 1024.0  # f32 in + dense i16 out + {scale, nnz} per 1024
HBM_PEAK_GBS = 8000.0             # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
F32_PEAK_TFLOPS = 157.3           # f32 vector peak with FMA = 2 flop (MI355X_MICROARCH.md)
F32_UNFUSED_TFLOPS = F32_PEAK_TFLOPS / 2.0  # separately rounded mul + add: one flop per issue slot
K1_KERNEL = "glc::k1::k_mdct_fwd_st<4, 2, 2, 4, 16, 16, 0, false>"   # name in rocprofv3's kernel trace (stereo segment loader, priority by distance from the barrier, 4 i-steps per fetch, 16 waves)
D1_KERNEL = "glc::k_imdct_apply<true, true, true> on the kept plan (first decode of a stream: + k_imdct_plan + k_imdct_order)"


def make_shard_pcm(np, rank, world):
    """Deterministic 16-tone chord per channel (tonal -> compressed frames), generated on the
    host in f64 and rounded to f32; each rank builds only its shard + halo."""
    import glc_amd
    from glc_amd import shard
    n_frames = FRAMES_PER_GPU * world
    L = n_frames * HOP                      # per-channel samples; gives exactly n_frames frames
    n_samples = L * CH
    plan = glc_amd.plan_encode(n_samples, CH)
    assert plan.n_frames == n_frames
    me = shard.plan_shards(n_frames, L, world)[rank]
    return chord(np, me.t0, me.t_count), me, n_samples


def chord(np, t0, t_count):
    rng = np.random.RandomState(7)
    t = (np.arange(t0, t0 + t_count, dtype=np.float64)) / SR
    x = np.zeros((t_count, CH), np.float64)
    for c in range(CH):
        freqs = rng.uniform(80.0, 8000.0, 16)
        phases = rng.uniform(0, 2 * np.pi, 16)
        for f, p in zip(freqs, phases):
            x[:, c] += 0.05 * np.sin(2 * np.pi * f * t + p)
    return x.astype(np.float32).reshape(-1)


DUMP_PAYLOAD_FRAMES = 3072  # payload rows in --dump-outputs: all 4096 would be exactly 64 MiB of float32


def record_arrays(np, records, rec_bytes, channels, n_payload=None):
    """The fixed-size frame records of include/glc.h as float32 arrays, every value exact and every
    shape fixed by the frame count alone: is_raw [frames], scale and nnz [frames, ch], and for a
    fixed, seeded sample of `n_payload` frames (all frames if None; their indices, ascending, in
    payload_frames) payload [sample, ch, 2048] as a reader of the record takes it: a compressed
    frame's dense quantised row in [0, 1024) and zeros after it, a raw frame's windowed i16 plane.
    Bytes the encoder leaves undefined (header padding, payload[c][1024:] of a compressed frame) are
    not read, so equal encodes give equal arrays."""
    hdr = rec_bytes - 2 * 2 * HOP * channels
    rec = np.ascontiguousarray(records, np.uint8).reshape(-1, rec_bytes)
    nf = rec.shape[0]
    frames = np.arange(nf)
    if n_payload is not None and n_payload < nf:
        frames = np.sort(np.random.RandomState(0).choice(nf, n_payload, replace=False))
    is_raw = rec[:, 0:4].copy().view(np.uint32)[:, 0] != 0
    head = rec[:, 8:8 + 8 * channels].copy()
    payload = np.ascontiguousarray(rec[frames, hdr:]).view(np.int16).reshape(-1, channels, 2 * HOP)
    payload[~is_raw[frames], :, HOP:] = 0
    return {"is_raw": is_raw.astype(np.float32),
            "scale": head.view(np.float32).reshape(-1, channels, 2)[:, :, 0].copy(),
            "nnz": head.view(np.uint32).reshape(-1, channels, 2)[:, :, 1].astype(np.float32),
            "payload_frames": frames.astype(np.float32),
            "payload": payload.astype(np.float32)}


def dump_outputs(np, out_dir, arrays):
    total = sum(a.nbytes for a in arrays.values())
    assert total <= 64_000_000, f"--dump-outputs: {total} bytes exceed the 64 MB budget"
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


SPINUP_STEPS = 500  # untimed, before the --warmup steps
DECODE_SPINUP_CALLS = 400  # untimed decode calls before the decode leg is timed


def launch_ranks(args):
    """`python bench.py --gpus N` as the driver calls it: this process has made no GPU call; it
    starts N fresh ranks under torch.distributed.run, relays rank 0's JSON line and exit code."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__),
           "--gpus", str(args.gpus), "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--spinup", str(args.spinup)]
    if args.full:
        cmd.append("--full")
    if args.no_cpu_baseline:
        cmd.append("--no-cpu-baseline")
    if args.lean:
        cmd.append("--lean")
    if args.dump_outputs:
        cmd += ["--dump-outputs", os.path.abspath(args.dump_outputs)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE)
    line = None
    for ln in p.stdout.decode("utf-8", "replace").splitlines():
        if ln.startswith('{"metric"'):
            line = ln
    if line is not None:
        sys.stdout.write(line + "\n")
        sys.stdout.flush()
    if p.returncode != 0 or line is None:
        sys.stderr.write(f"bench.py: the {args.gpus}-rank run failed (rc {p.returncode})\n")
        raise SystemExit(p.returncode or 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="also every measurement beside the headline (rooflines, other rates, decode, host boundary, CPU baseline, checks)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--lean", action="store_true",
                    help="with --full: only the timed steps and the K1 leg (profiling runs: no other rates, decode, host boundary, CPU baseline, child process)")
    ap.add_argument("--spinup", type=int, default=SPINUP_STEPS,
                    help="untimed steps before --warmup that bring the device clock up after the idle set-up phase")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write rank 0's frame records of the last timed step to DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.lean and not args.full:
        ap.error("--lean narrows --full; pass both")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return launch_ranks(args)
    # The contract is ONE JSON line on stdout.  Native libraries write there too (RCCL prints a
    # version banner to stdout when the first communicator is created), so everything written to
    # fd 1 during the run is sent to stderr and the JSON line goes to the saved descriptor.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    import numpy as np
    import torch
    import torch.distributed as dist

    import glc_amd
    from glc_amd import shard

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: required by RCCL on this host driver
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    assert torch.cuda.is_available(), "bench.py needs a GPU (the product has no CPU fallback)"
    ndev = torch.cuda.device_count()
    # The real run is one rank per GPU over nccl = RCCL.  On a box with fewer GPUs than ranks (the
    # one-GPU development box) the ranks share devices and the gather goes through host memory
    # (gloo): a rehearsal of the N > 1 code path, labelled as such in the output.
    backend = os.environ.get("GLC_BENCH_BACKEND", "nccl" if ndev >= world else "gloo")
    if backend != "nccl" or ndev <= local_rank:
        local_rank = local_rank % ndev
    torch.cuda.set_device(local_rank)
    # GLC_BENCH_FORCE_DIST=1 takes the collective path even with one rank: the only way to
    # rehearse RCCL itself on a one-GPU box
    dist_on = world > 1 or os.environ.get("GLC_BENCH_FORCE_DIST") == "1"
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    # ---- inputs resident in HBM before the timed region --------------------------------
    pcm_host, me, n_samples = make_shard_pcm(np, rank, world)
    d_pcm = torch.from_numpy(pcm_host).cuda()
    rec_bytes = glc_amd.lib.glc_record_bytes(CH)
    d_rec = torch.empty(me.n_frames * rec_bytes, dtype=torch.uint8, device="cuda")
    d_coef = torch.empty((me.n_frames * CH, 1024), dtype=torch.float32, device="cuda")
    blob_cap = glc_amd.compact_bound(CH, me.n_frames)
    d_blob = torch.empty(blob_cap, dtype=torch.uint8, device="cuda")
    enc = glc_amd.Encoder(SR, device=local_rank)  # owns the HIP stream its kernels run on
    torch.cuda.synchronize()

    def step():
        enc.encode_range_device(d_pcm.data_ptr(), me.t0, me.t_count, n_samples, CH,
                                me.frame_begin, me.frame_end, d_rec.data_ptr())

    def barrier():
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        enc.synchronize()

    def gather_once():
        """The job's single gather: compact this rank's records on the device, send the blob."""
        info = enc.compact_device_records(d_rec.data_ptr(), me.n_frames, CH, d_blob.data_ptr(), blob_cap)
        blob = d_blob[:info.bytes]
        got = shard.gather_compact(blob if backend == "nccl" else blob.cpu())
        torch.cuda.synchronize()
        return info, got

    # clocks: the device idles at a low DVFS state and needs some tens of milliseconds of load to
    # settle; a short spin-up (reported in config) keeps small --steps runs comparable to long ones
    if dist_on:
        step()
        enc.synchronize()
        gather_once()        # untimed: communicator / buffers of the collective exist before the clock starts
    for _ in range(args.spinup):   # after the collective's set-up, which lets the device clock down
        step()
    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    enc.synchronize()
    torch.cuda.synchronize()
    t_steps = time.perf_counter() - t0
    info = blobs = None
    if dist_on:
        info, blobs = gather_once()
    elapsed = time.perf_counter() - t0
    if dist_on:
        tt = torch.tensor([elapsed, t_steps], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed, t_steps = float(tt[0].item()), float(tt[1].item())
    barrier()
    if args.dump_outputs and rank == 0:   # before any later leg writes d_rec again
        dump_outputs(np, args.dump_outputs, record_arrays(np, d_rec.cpu().numpy(), rec_bytes, CH,
                                                                  DUMP_PAYLOAD_FRAMES))

    samples_per_step = FRAMES_PER_GPU * HOP * CH * world
    value = samples_per_step * args.steps / elapsed / 1e6

    # ---- the gather's sizes; with --full, the gathered blobs assemble into one valid stream (rank 0)
    gather = None
    if dist_on:
        gather = {"ms": round((elapsed - t_steps) * 1e3, 3),
                  "in_timed_region": True,
                  "value_excluding_gather": round(samples_per_step * args.steps / t_steps / 1e6, 2),
                  "backend": "nccl (RCCL over xGMI)" if backend == "nccl"
                  else f"{backend} (rehearsal: {world} ranks on {ndev} GPU(s), blobs through host memory)",
                  "what": "per rank: device compaction of its 4096 records (scan + ballot pack) + size exchange "
                          "(8 B per rank) + one gather of the compact blobs to rank 0"}
        if rank == 0:
            sizes = [int(b.numel()) for b in blobs]
            gather["bytes_to_root"] = int(sum(sizes[1:]))
            gather["dense_record_bytes_to_root"] = int(rec_bytes * FRAMES_PER_GPU * (world - 1))
        if rank == 0 and args.full:
            ea = shard.assemble_frame_shards(blobs, SR, n_samples, CH)
            gather["assembled_frames"] = int(ea.info().n_frames)
            gather["assembled_raw_frames"] = int(ea.info().n_raw_frames)
            assert gather["assembled_frames"] == FRAMES_PER_GPU * world
            # the assembled .glc equals a single-rank encode of the same stream (rehearsal sizes only:
            # the root re-generates and re-encodes the WHOLE stream for this)
            verify = os.environ.get("GLC_BENCH_VERIFY", "1" if world <= 2 else "0") == "1"
            gather["assembled_equals_single_rank"] = None
            if verify:
                whole = chord(np, 0, FRAMES_PER_GPU * world * HOP)
                single = enc.encode(whole, CH)
                gather["assembled_equals_single_rank"] = bool(single.to_bytes() == ea.to_bytes())
                assert gather["assembled_equals_single_rank"], "gathered stream differs from the single-rank encode"
                del whole, single

    out = {
        "metric": "Msamples/s encoded (48 kHz stereo batch) at 1/2/4/8 GPUs; % HBM roofline",
        "value": round(value, 2),
        "unit": "Msamples/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": "BASELINE configs[1]: batch-encode 4096 frames x 1024 samples, "
                               "48 kHz stereo synthetic PCM (16-tone chord per channel) per GPU",
                   "frames_per_gpu": FRAMES_PER_GPU, "channels": CH, "sample_rate": SR,
                   "samples_per_step": samples_per_step,
                   "sharding": f"frame-range x{world}" + (", one gather of the compact blobs at the end "
                                                           "(inside the timed region)" if dist_on else ""),
                   "spinup_steps": args.spinup},
        "gather": gather,
    }
    if not args.full:
        if rank == 0:
            sys.stdout.flush()
            os.write(real_stdout, (json.dumps(out) + "\n").encode())
        if dist_on:
            dist.destroy_process_group()
        return

    # ---- dominant kernel (K1, forward MDCT) timed alone with events on ITS stream -------
    k1_reps = max(10, min(args.steps, 50))

    def k1():
        enc.mdct_forward_device(d_pcm.data_ptr(), me.t0, me.t_count, n_samples, CH, me.frame_begin,
                                me.frame_end, d_coef.data_ptr())

    import ctypes as C
    L = glc_amd.lib
    L.glc_debug_clock_probe_begin.restype = C.c_int
    L.glc_debug_clock_probe_begin.argtypes = [C.c_void_p, C.c_uint32]
    L.glc_debug_clock_probe_end.restype = C.c_int
    L.glc_debug_clock_probe_end.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    for _ in range(args.spinup if dist_on else 10):   # (the gather and its host-side assembly let the device clock down)
        step()
    k1()
    # the clock the chip HOLDS under this kernel: one sleeping wave reads the shader-cycle counter against
    # the 100 MHz reference over ~60 % of the timed launches (include/glc_debug.h; measurement only)
    probe_ok = (not args.lean) and L.glc_debug_clock_probe_begin(enc._h, int(0.6 * k1_reps * 550)) == 0
    enc.timer_begin()          # HIP events on the stream the kernels are launched on
    for _ in range(k1_reps):
        k1()
    k1_ms = enc.timer_end() / k1_reps
    k1_clock_ghz = None
    if probe_ok:
        g = C.c_float()
        if L.glc_debug_clock_probe_end(enc._h, C.byref(g)) == 0 and 0.3 < g.value < 3.5:
            k1_clock_ghz = float(g.value)
    # the same launches through the kernel this one replaced (k_mdct_fwd_dma, round 3's first half), pinned with
    # glc_debug_set_mdct_variant: same process, same buffers, same probe - reported beside, never as `value`
    k1_prev = None
    if not args.lean and not dist_on:
        L.glc_debug_set_mdct_variant.restype = C.c_int
        L.glc_debug_set_mdct_variant.argtypes = [C.c_void_p, C.c_int]
        if L.glc_debug_set_mdct_variant(enc._h, 1) == 0:
            for _ in range(5):
                k1()
            pv_probe = L.glc_debug_clock_probe_begin(enc._h, int(0.6 * k1_reps * 580)) == 0
            enc.timer_begin()
            for _ in range(k1_reps):
                k1()
            pv_ms = enc.timer_end() / k1_reps
            pv_ghz = None
            if pv_probe:
                g = C.c_float()
                if L.glc_debug_clock_probe_end(enc._h, C.byref(g)) == 0 and 0.3 < g.value < 3.5:
                    pv_ghz = float(g.value)
            assert L.glc_debug_set_mdct_variant(enc._h, 0) == 0
            k1_prev = {"kernel": "glc::k1::k_mdct_fwd_dma<4, 2, 1, false> (128x128 tile, both operands from LDS)",
                       "ms_per_launch": round(pv_ms, 4), "clock_ghz_held": round(pv_ghz, 3) if pv_ghz else None,
                       "shipped_over_previous": round(pv_ms / k1_ms, 4)}
            for _ in range(5):
                k1()
    enc.timer_begin()          # whole step with events too (profile cross-check)
    for _ in range(k1_reps):
        step()
    step_ev_ms = enc.timer_end() / k1_reps

    samples_per_launch = FRAMES_PER_GPU * HOP * CH  # per GPU
    k1_tflops = samples_per_launch * FLOP_PER_SAMPLE / (k1_ms * 1e-3) / 1e12
    k1_gbs = samples_per_launch * BYTES_PER_SAMPLE / (k1_ms * 1e-3) / 1e9

    # ---- the north_star's 44.1 / 96 kHz variants of the same batch (only the band tables of the
    # quantiser depend on the rate; reported beside the headline, never as `value`) ------------
    other_rates = {}
    for sr2 in (() if args.lean else (44100, 96000)):
        e2 = glc_amd.Encoder(sr2, device=local_rank)
        reps = max(10, min(args.steps, 50))
        for _ in range(args.spinup):  # the device clocked down while the host built this rate's tables
            e2.encode_range_device(d_pcm.data_ptr(), me.t0, me.t_count, n_samples, CH, me.frame_begin,
                                   me.frame_end, d_rec.data_ptr())
        e2.timer_begin()
        for _ in range(reps):
            e2.encode_range_device(d_pcm.data_ptr(), me.t0, me.t_count, n_samples, CH, me.frame_begin,
                                   me.frame_end, d_rec.data_ptr())
        ms = e2.timer_end() / reps
        ms_all = [ms]
        if dist_on:  # every rank times its own shard; the job's rate is all samples over the slowest rank
            tt = torch.tensor([ms], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
            gl = [torch.zeros_like(tt) for _ in range(world)]
            dist.all_gather(gl, tt)
            ms_all = [float(t.item()) for t in gl]
        other_rates[str(sr2)] = {"Msamples/s": round(FRAMES_PER_GPU * HOP * CH * world / (max(ms_all) * 1e-3) / 1e6, 1),
                                 "ms_per_step_events": round(max(ms_all), 4),
                                 "ms_per_step_events_min_over_ranks": round(min(ms_all), 4)}
        e2.close()
    other_rates = other_rates or None
    # restore the 48 kHz records for the checks below
    step()
    enc.synchronize()
    # K1's event time and held clock on every rank (min / max over ranks)
    k1_ranks = None
    if dist_on:
        tt = torch.tensor([k1_ms, k1_clock_ghz or 0.0], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        gl = [torch.zeros_like(tt) for _ in range(world)]
        dist.all_gather(gl, tt)
        ks = [float(t[0].item()) for t in gl]
        cs = [float(t[1].item()) for t in gl if float(t[1].item()) > 0]
        k1_ranks = {"ms_per_launch_min": round(min(ks), 4), "ms_per_launch_max": round(max(ks), 4),
                    "clock_ghz_min": round(min(cs), 3) if cs else None, "clock_ghz_max": round(max(cs), 3) if cs else None}

    # ---- sanity: records of this run assemble into a valid stream (rank 0, own shard) ----
    encoded = None
    if rank == 0 and not args.lean:
        # (rank 0's 4096 records, indexed as a stream of their own: the bookkeeping below is per GPU)
        ea = glc_amd.EncodedAudio.from_records(SR, FRAMES_PER_GPU * HOP * CH, CH, d_rec.cpu().numpy())
        i = ea.info()
        cinfo = enc.compact_device_records(d_rec.data_ptr(), me.n_frames, CH, d_blob.data_ptr(), blob_cap)
        encoded = {"n_frames": int(i.n_frames), "raw_frames": int(i.n_raw_frames), "total_nnz": int(i.total_nnz),
                   "glc_bytes": int(glc_amd.lib.glc_serialized_size(ea._h)),
                   "compact_blob_bytes": int(cinfo.bytes), "dense_record_bytes": int(rec_bytes * me.n_frames)}

    # ---- PCIe-inclusive host boundary (Encoder::encode from host memory + save_encoded bytes);
    # reported beside the headline, never as `value` -------------------------------------------
    host_boundary = None
    if rank == 0 and not args.lean:
        best = None
        ea_h = blob = None
        for _ in range(60):  # the device clocked down while the records came back to the host: 75 ms of the same call
            ea_h = enc.encode(pcm_host, CH)
            del ea_h
        ea_h = None
        for _ in range(8):
            # the previous result is dropped first, as a caller encoding file after file would: with two
            # EncodedAudio alive the allocator hands out fresh pages and the call pays their page faults
            del ea_h, blob
            h0 = time.perf_counter()
            ea_h = enc.encode(pcm_host, CH)
            h1 = time.perf_counter()
            blob = ea_h.to_bytes()
            h2 = time.perf_counter()
            if best is None:
                best = [h1 - h0, h2 - h1, len(blob)]
            best[0] = min(best[0], h1 - h0)   # each leg its own best-of
            best[1] = min(best[1], h2 - h1)
        pcm_bytes = pcm_host.size * 4
        # the same call through the reference's own data model (nested vectors): tools/bridge_bench.cpp, a
        # C++ process of its own driving the structured bridge of include/glc.h like the Rust shim of
        # INTEGRATION.md section 3 would; this process is idle meanwhile
        shim = None
        exe = os.path.join(ROOT, "build", "bridge_bench")
        if os.path.exists(exe):
            try:
                np.asarray(pcm_host[:FRAMES_PER_GPU * HOP * CH]).tofile(os.path.join(ROOT, "build", "chord_cfg2.f32"))
                r = subprocess.run([exe, str(FRAMES_PER_GPU), str(CH), str(SR)], cwd=ROOT, capture_output=True, text=True, timeout=300)
                for ln in r.stdout.splitlines():
                    if ln.startswith("summary_json "):
                        shim = json.loads(ln[len("summary_json "):])
                if shim is None:
                    shim = {"error": (r.stdout + r.stderr)[-300:]}
            except Exception as e:  # noqa: BLE001 - a measurement beside the headline must not fail the bench
                shim = {"error": repr(e)}
        host_boundary = {"encode_ms": round(best[0] * 1e3, 3), "serialize_ms": round(best[1] * 1e3, 3),
                         "Msamples/s": round(FRAMES_PER_GPU * HOP * CH / best[0] / 1e6, 1), "glc_bytes": best[2],
                         "h2d_bytes": int(pcm_bytes),
                         "pcie_gen5_x16_GBs": 63.0,
                         "h2d_floor_ms_at_pcie_peak": round(pcm_bytes / 63.0e9 * 1e3, 3),
                         "shim_equivalent": shim,
                         "note": "host f32 PCM (pageable, caller-owned) -> four 1024-frame rounds on two streams through a "
                                 "three-thread pipeline: round i+1 goes up under round i's kernels, round i-1's compact blob "
                                 "comes down and is indexed meanwhile; the payload lands in the EncodedAudio pools directly; "
                                 "encode_ms and serialize_ms are each the best of 8.  shim_equivalent: the calls a Rust "
                                 "Encoder::encode / Decoder::decode make through the structured bridge, with the "
                                 "EncodedAudio as nested vectors on the host side (tools/bridge_bench.cpp)"}

    # ---- decode of the same batch, device-resident (sparse rows resident -> interleaved PCM in
    # HBM): D1 sparse IMDCT + window, D2 overlap-add.  Beside the headline, never `value`. ---------
    decode = None
    if rank == 0 and not args.lean:
        ea_d = glc_amd.EncodedAudio.from_records(SR, FRAMES_PER_GPU * HOP * CH, CH, d_rec.cpu().numpy())
        dec = glc_amd.Decoder(CH, SR, device=local_rank)
        d_all = torch.empty((FRAMES_PER_GPU + 1) * HOP * CH, dtype=torch.float32, device="cuda")
        d_blk = torch.empty((FRAMES_PER_GPU * CH, 2048), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        reps = max(20, min(args.steps, 100))
        t_u0 = time.perf_counter()
        dec.decode_device(ea_d, d_all.data_ptr(), d_all.numel())   # first call: row prep + upload
        dec.synchronize()
        first_ms = (time.perf_counter() - t_u0) * 1e3
        # the device clocked down while the host built the EncodedAudio: bring it back up first (the
        # same reason as SPINUP_STEPS for the encode; 400 calls = 45 ms)
        for _ in range(DECODE_SPINUP_CALLS):
            dec.decode_device(ea_d, d_all.data_ptr(), d_all.numel())
        dec.synchronize()
        t_d0 = time.perf_counter()
        for _ in range(reps):
            dec.decode_device(ea_d, d_all.data_ptr(), d_all.numel())
        dec.synchronize()
        d_ms = (time.perf_counter() - t_d0) * 1e3 / reps
        for _ in range(20):
            dec.imdct_device(ea_d, 0, FRAMES_PER_GPU, d_blk.data_ptr())
        d1_probe = L.glc_debug_clock_probe_begin(dec._h, int(0.6 * reps * 70)) == 0   # ~70 us per launch
        dec.timer_begin()
        for _ in range(reps):
            dec.imdct_device(ea_d, 0, FRAMES_PER_GPU, d_blk.data_ptr())
        d1_ms = dec.timer_end() / reps
        d1_clock = None
        if d1_probe:
            g = C.c_float()
            if L.glc_debug_clock_probe_end(dec._h, C.byref(g)) == 0 and 0.3 < g.value < 3.5:
                d1_clock = float(g.value)
        total_nnz = int(ea_d.info().total_nnz)
        nnz_row = total_nnz / (FRAMES_PER_GPU * CH)
        d1_tflops = total_nnz * 2048.0 * 2.0 / (d1_ms * 1e-3) / 1e12
        decode = {"Msamples/s": round(FRAMES_PER_GPU * HOP * CH / (d_ms * 1e-3) / 1e6, 1), "ms": round(d_ms, 4),
                  "first_call_ms": round(first_ms, 3), "nnz_per_row": round(nnz_row, 1),
                  "roofline": {"bound": "valu", "kernel": D1_KERNEL, "achieved": round(d1_tflops, 3),
                               "peak": F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(d1_tflops / F32_PEAK_TFLOPS, 4),
                               "frac_of_unfused_ceiling": round(d1_tflops / F32_UNFUSED_TFLOPS, 4),
                               "clock_ghz_held": round(d1_clock, 3) if d1_clock else None,
                               "frac_of_unfused_ceiling_at_held_clock":
                                   round(d1_tflops / (F32_UNFUSED_TFLOPS * d1_clock / 2.4), 4) if d1_clock else None,
                               "ms_per_launch": round(d1_ms, 4),
                               "flop": "2 x 2048 x stored non-zeros (adding the +0.0 products of absent "
                                       "coefficients is the identity, so they are not work)"},
                  "note": "glc_decode_device per call with the stream's sparse rows already resident on the device "
                          "(D1 + D2, wall clock); first_call_ms includes the one-off row preparation + upload"}
        dec.close()

    # ---- CPU baseline: the oracle (a port of src/codec.rs) on this box's cores, rank 0, N=1
    cpu = None
    if rank == 0 and not args.no_cpu_baseline and not args.lean:
        from oracle import oracle as O  # checker/baseline only — never on the product path
        cores = min(16, os.cpu_count() or 1)  # a one-GPU box's CPU share is 16 cores (the other ranks idle in the barrier below)
        nfr = FRAMES_PER_GPU  # the full cfg2 batch, timed twice (~15 core-seconds of CPU work)
        sec = min(O.time_encode_frames(pcm_host, SR, CH, 0, nfr, n_threads=cores) for _ in range(2))
        cpu = {"value": round(nfr * HOP * CH / sec / 1e6, 3), "unit": "Msamples/s", "cores": cores,
               "kind": "port",
               "sample": f"all {nfr} frames of the same 48 kHz stereo batch, best of 2 passes, {cores} threads "
                         f"({sec:.2f} s wall); C restatement of src/codec.rs (no Rust toolchain in the image)"}

    # HBM-side traffic of K1 comes from PMC counters (separate rocprofv3 --pmc passes over this same
    # command, summarised by tools/pmc_traffic.py into profiles/): it cannot be measured from inside
    # the run, so the line names the file and the commit it was taken at.
    traffic = traffic_source = None
    tpath = os.path.join(ROOT, "profiles", "k1_traffic.json")
    if os.path.exists(tpath):
        try:
            tj = json.load(open(tpath))
            traffic = tj.get("hbm_bytes_per_launch")
            traffic_source = f"profiles/k1_traffic.json @{tj.get('commit', 'unknown')} ({tj.get('method', 'pmc')})"
        except Exception:
            traffic = None

    if dist_on:
        dist.barrier()   # rank 0's single-rank legs (decode, host boundary, CPU baseline) are done
    if rank == 0:
        k1_peak_held = F32_PEAK_TFLOPS * k1_clock_ghz / 2.4 if k1_clock_ghz else None
        out["config"]["decode_spinup_calls"] = DECODE_SPINUP_CALLS
        out.update({
            "roofline": {"bound": "valu", "kernel": K1_KERNEL, "achieved": round(k1_tflops, 3),
                         "peak": F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(k1_tflops / F32_PEAK_TFLOPS, 4),
                         "frac_of_unfused_ceiling": round(k1_tflops / F32_UNFUSED_TFLOPS, 4),
                         "clock_ghz_held": round(k1_clock_ghz, 3) if k1_clock_ghz else None,
                         "peak_at_held_clock": round(k1_peak_held, 1) if k1_peak_held else None,
                         "frac_at_held_clock": round(k1_tflops / k1_peak_held, 4) if k1_peak_held else None,
                         "frac_of_unfused_ceiling_at_held_clock": round(2.0 * k1_tflops / k1_peak_held, 4) if k1_peak_held else None,
                         "traffic": traffic, "traffic_source": traffic_source,
                         "traffic_is": "bytes that missed the XCD L2s (FETCH_SIZE / WRITE_SIZE per launch, each access pattern of the "
                                       "kernel corrected by the factor measured for it on known byte counts: dwordx4 reads count "
                                       "half, scalar loads and stores whole); the 16 MiB working set of a step is Infinity-Cache "
                                       "resident, so these are L2-fabric bytes, an upper bound on HBM bytes",
                         "ms_per_launch": round(k1_ms, 4), "per_rank": k1_ranks, "previous_kernel": k1_prev,
                         "note": "f32 vector-ALU issue roofline (157.3 TFLOP/s at 2.4 GHz counts an FMA as 2 flop); 4096 "
                                 "flop/sample = 2048 separately rounded mul + 2048 add.  Bit-exact parity forbids "
                                 "FMA and MFMA accumulation, so the ceiling of this kernel is 78.65 TFLOP/s "
                                 "(frac_of_unfused_ceiling).  clock_ghz_held: shader clock measured in-kernel beside "
                                 "these launches (s_memtime / s_memrealtime); the *_at_held_clock fractions scale "
                                 "the peak by it."},
            "roofline_hbm": {"bound": "hbm", "achieved": round(k1_gbs, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": round(k1_gbs / HBM_PEAK_GBS, 5), "pct_hbm_roofline": round(100 * k1_gbs / HBM_PEAK_GBS, 3),
                             "note": "BASELINE metric's '% HBM roofline': 6.006 algorithmic B/sample; the "
                                     "path is compute-bound (SURVEY F4), cap under parity = 1.44 %"},
            "cpu_baseline": cpu,
            "vs_cpu_baseline": round(value / cpu["value"], 1) if cpu else None,
            "step_ms_events": round(step_ev_ms, 4),
            "other_sample_rates": other_rates,
            "host_boundary": host_boundary,
            "decode": decode,
            "encoded": encoded,
        })
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    if dist_on:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
