"""Build-time guard of the numerics contract: the transform kernels must not contain a fused
multiply-add (v_fma*, v_fmac*, v_pk_fma*, v_mad*, v_mac*, v_dot*) or an accumulating MFMA — the
reference accumulates with a separately rounded multiply and add.

  k_mdct_fwd_sched / k_mdct_fwd_dma / k_mdct_fwd_st / k_mdct_fwd_small / k_mdct_fwd_small_rows / k_mdct_edge_rows /
  k_imdct_apply  strict: no fused op at all (no division or sqrt inside)
  k_mdct_edge_rows (the edge transform: k_mdct_fwd_small_rows' chain with the row list taken from the kernel arguments)
                must hold exactly the v_pk_mul_f32 and v_pk_add_f32 of k_mdct_fwd_small_rows - one body, one chain: 8
                blocks of 16 i-steps, a packed multiply and a packed add per i-step and pair of rows, 128 each at the
                least - and, like it, no spill and no v_pk_fma_f32
  k_mdct_edge_rows_capped (the same body with a ring of 4 blocks)   half of those counts, 64 each at the least, no spill,
                no v_pk_fma_f32, and - from the code object's metadata - at most 192 VGPRs and 24576 bytes of LDS: what
                a CU has left beside two resident workgroups of the screened quantiser (2 x 160 registers per SIMD, 2 x
                69632 bytes)
  k_imdct_rows / k_imdct_plan   fused ops allowed only inside hipcc's correctly-rounded f32 division expansion
                (v_div_scale ... v_div_fixup), which the raw-frame path `i16 / 32767.0` needs
  k_mdct_mix_st (the mixed-role form of k_mdct_fwd_st)   v_pk_fma_f32 alone is allowed: its bound waves
                accumulate an upper bound with it, never a coefficient; its exact waves run k_mdct_fwd_st's own multiply /
                add block.  The i loop exists once per role - exact, bound, bound + A of row 0 / 1 / 2 / 3 and, in the
                instantiations with E > 0 exact pairs per hybrid wave (the third template argument), hybrid - each copy
                BK = 16 i-steps of 16 packed multiply-adds (a lane's 4 rows x 4 column pairs).  A hybrid copy holds
                64 (4 - E) v_pk_fma_f32 and 64 E each of v_pk_mul_f32 and v_pk_add_f32.  Every instantiation may hold at
                most 5 x 256 + 64 (4 - E) v_pk_fma_f32 (E = 0: 5 x 256) and must hold 256 + 64 E v_pk_mul_f32 and as many
                v_pk_add_f32, so a fused op in an exact pair shows here as well as in the bit-exact parity of
                tests/test_encode_screen.py and tests/test_encode_balance.py
  k_mdct_mx_st (the matrix form of the mixed-role transform)   v_mfma_f32_*_bf16 alone is allowed: its
                matrix waves accumulate the upper bound with it, never a coefficient.  No v_pk_fma_f32 at all: the bound has
                left the vector ALU.  Its exact waves run k_mdct_fwd_st's multiply / add block on a lane's 2 rows x 8
                columns: the one copy of their i loop holds BK = 16 i-steps of 8 packed multiplies and 8 packed adds, so
                every instantiation must hold at least 128 v_pk_mul_f32 and as many v_pk_add_f32.
The quantiser / decision / overlap-add kernels are not scanned: their IEEE divide, sqrt and
64-bit index division expand to FMA-based sequences by design.  The arithmetic of the quantiser and the
raw-or-compressed decision is pinned instead by tests/test_quantizer_edges.py, which drives them with
coefficient rows sitting on every decision edge (thresholds, noise floor, peak gate, rounding, the raw
flip point); the overlap-add by the bit-exact parity tests."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gapless-lossy-codec_amd", "csrc")
ISA = os.path.join(ROOT, "build", "isa", "glc_kernels-hip-amdgcn-amd-amdhsa-gfx950.s")
FORBIDDEN = re.compile(r"^\s+(v_fma\w*|v_fmac\w*|v_pk_fma\w*|v_mad_\w*f32|v_mac\w*|v_dot\w*|v_mfma\w*)\b")
KERNELS = ("k_mdct_fwd_sched", "k_mdct_fwd_dma", "k_mdct_fwd_st", "k_mdct_mix_st", "k_mdct_mx_st", "k_mdct_fwd_small_rows", "k_mdct_edge_rows_capped", "k_mdct_edge_rows", "k_mdct_fwd_small", "k_imdct_rows", "k_imdct_plan", "k_imdct_apply")
DIV_WINDOW = {"k_imdct_rows", "k_imdct_plan"}
BOUND_FMA = re.compile(r"^\s+v_pk_fma_f32\b")  # the one fused op of k_mdct_mix_st's bound waves
MIX_LOOP_MACS = 16 * 16  # packed multiply-adds in one copy of k_mdct_mix_st's i loop: BK i-steps x (4 rows x 8 columns / 2)
MIX_BOUND_COPIES = 5     # bound, bound + A of row 0 .. 3
MX_MFMA = re.compile(r"^\s+v_mfma_f32_\w+_bf16\b")  # the one matrix op of k_mdct_mx_st's matrix waves
MX_LOOP_MACS = 16 * 8  # packed multiplies (and adds) in the exact waves' i loop: BK i-steps x (2 rows x 8 columns / 2)
EDGE_CAP_VGPRS, EDGE_CAP_LDS = 192, 24576  # k_mdct_edge_rows_capped, from the metadata
ROWS_LOOP_MACS = 8 * 16  # packed multiplies (and adds) of the latency chain's loop body: 8 blocks x 16 i-steps, a pair of rows
MIX_NAME = re.compile(r"k_mdct_mix_stILi\d+ELi\d+ELi([0-3])EE")  # <MINW, CH, E>


def mix_bounds(name):
    """(v_pk_fma_f32 at most, v_pk_mul_f32 / v_pk_add_f32 at least) of an instantiation, from the E in its name."""
    e = int(MIX_NAME.search(name).group(1))
    per_pair = MIX_LOOP_MACS // 4      # one column pair of a copy: 16 i-steps x 4 rows
    return MIX_BOUND_COPIES * MIX_LOOP_MACS + (per_pair * (4 - e) if e else 0), MIX_LOOP_MACS + per_pair * e


def main() -> int:
    subprocess.check_call(["make", "-C", CSRC, "-s", "isa"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    cur, bad, seen, in_div = None, [], set(), False
    first_ds = {}   # kernel -> True once its first ds_read has been seen
    mx = {}         # instantiation of k_mdct_mx_st -> [v_mfma_f32_*_bf16, v_pk_mul_f32, v_pk_add_f32] counts
    rows = {"k_mdct_fwd_small_rows": [0, 0], "k_mdct_edge_rows": [0, 0], "k_mdct_edge_rows_capped": [0, 0]}
    meta, meta_cur = {}, None  # kernel of the metadata section -> {field: value}  # [v_pk_mul_f32, v_pk_add_f32] counts
    mix = {}        # instantiation of k_mdct_mix_st -> [v_pk_fma_f32, v_pk_mul_f32, v_pk_add_f32] counts
    for line in open(ISA):
        mm = re.match(r"^\s+\.(name|vgpr_count|group_segment_fixed_size|vgpr_spill_count):\s+(\S+)", line)
        if mm:  # (a kernel's fields come in alphabetical order: group_segment_fixed_size in front of its name)
            if mm.group(1) == "group_segment_fixed_size":
                meta_cur = {"lds": int(mm.group(2))}
            elif mm.group(1) == "name" and meta_cur is not None:
                meta[mm.group(2)] = meta_cur
            elif meta_cur is not None and mm.group(1) != "name":
                meta_cur[mm.group(1)] = int(mm.group(2))
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = next((k for k in KERNELS if k in m.group(1)), None)
            cur_mix = mix.setdefault(m.group(1), [0, 0, 0]) if cur == "k_mdct_mix_st" else None
            cur_mx = mx.setdefault(m.group(1), [0, 0, 0]) if cur == "k_mdct_mx_st" else None
            in_div = False
            first_ds = {}
            if cur:
                seen.add(cur)
        elif cur and cur in DIV_WINDOW and "v_div_scale_f32" in line:
            in_div = True
        elif cur and "v_div_fixup_f32" in line:
            in_div = False
        elif cur and FORBIDDEN.match(line) and not in_div and not (cur == "k_mdct_mix_st" and BOUND_FMA.match(line)) \
                and not (cur == "k_mdct_mx_st" and MX_MFMA.match(line)):
            bad.append((cur, line.strip()))
        # k_mdct_fwd_small waits for its LDS operands with COUNTED lgkmcnt (LDS returns in order): a scalar
        # load in flight at the same time would make those counts meaningless (SMEM returns out of order)
        if cur == "k_mdct_fwd_small":
            if re.match(r"^\s+ds_read", line):
                first_ds[cur] = True
            elif first_ds.get(cur) and re.match(r"^\s+(s_load|s_buffer_load)", line):
                bad.append((cur, "scalar load beside counted LDS waits: " + line.strip()))
        asm_async = cur and (cur.startswith("k_mdct_") or cur == "k_imdct_apply")  # loads issued and waited for in separate asm statements
        if asm_async and re.match(r"^\s+(scratch_|buffer_store.*offen.*s\[0:3\]|buffer_load.*off.*s\[0:3\])", line):
            bad.append((cur, "register spill: " + line.strip()))
        # k_mdct_fwd_st / k_imdct_apply keep table values / records in SGPRs that an asm statement loads and a LATER
        # one waits for: a spill into VGPR lanes between the two copies stale values (it happened in a tuning
        # variant: wrong results and a memory fault), besides putting v_writelane / v_readlane into the inner loop
        if asm_async and re.match(r"^\s+(v_writelane|v_readlane)", line):
            bad.append((cur, "scalar register spill: " + line.strip()))
        if cur in rows:
            pk = re.match(r"^\s+v_pk_(mul|add)_f32\b", line)
            if pk:
                rows[cur][("mul", "add").index(pk.group(1))] += 1
        if cur == "k_mdct_mix_st":
            pk = re.match(r"^\s+v_pk_(fma|mul|add)_f32\b", line)
            if pk:
                cur_mix[("fma", "mul", "add").index(pk.group(1))] += 1
        if cur == "k_mdct_mx_st":
            if MX_MFMA.match(line):
                cur_mx[0] += 1
            pk = re.match(r"^\s+v_pk_(mul|add)_f32\b", line)
            if pk:
                cur_mx[1 + ("mul", "add").index(pk.group(1))] += 1
        if line.startswith(".Lfunc_end"):  # (not s_endpgm: a kernel with an early return has blocks behind its first one)
            cur = None
    missing = set(KERNELS) - seen
    if missing:
        print("check_isa: kernels not found in ISA:", sorted(missing))
        return 1
    for name, (n_fma, n_mul, n_add) in mix.items():
        if not MIX_NAME.search(name):
            bad.append(("k_mdct_mix_st", f"{name}: no <MINW, CH, E> in the name"))
            continue
        fma_max, mul_min = mix_bounds(name)
        if n_fma > fma_max or n_mul < mul_min or n_add < mul_min:
            bad.append(("k_mdct_mix_st", f"{name}: {n_fma} v_pk_fma_f32 (at most {fma_max}: the bound copies and the hybrid copy's bound pairs), "
                                         f"{n_mul} v_pk_mul_f32 / {n_add} v_pk_add_f32 (at least {mul_min} each: the exact copy and the hybrid copy's exact pairs)"))
    for name, (n_mfma, n_mul, n_add) in mx.items():
        if not n_mfma or n_mul < MX_LOOP_MACS or n_add < MX_LOOP_MACS:
            bad.append(("k_mdct_mx_st", f"{name}: {n_mfma} v_mfma_f32_*_bf16 (the bound must be on the matrix pipe), {n_mul} v_pk_mul_f32 / "
                                        f"{n_add} v_pk_add_f32 (at least {MX_LOOP_MACS} each: the exact waves' i loop)"))
    if rows["k_mdct_edge_rows"] != rows["k_mdct_fwd_small_rows"] or min(rows["k_mdct_edge_rows"]) < ROWS_LOOP_MACS:
        bad.append(("k_mdct_edge_rows", f"{rows['k_mdct_edge_rows']} v_pk_mul_f32 / v_pk_add_f32, k_mdct_fwd_small_rows has "
                                        f"{rows['k_mdct_fwd_small_rows']} (equal, and at least {ROWS_LOOP_MACS} each: one chain)"))
    # (the chain's packed operations halve with the ring; the packed multiplies of the staging - rows times window - stay)
    n_mul, n_add = rows["k_mdct_fwd_small_rows"]
    half = [n_mul - n_add + n_add // 2, n_add // 2]
    if rows["k_mdct_edge_rows_capped"] != half or min(rows["k_mdct_edge_rows_capped"]) < ROWS_LOOP_MACS // 2:
        bad.append(("k_mdct_edge_rows_capped", f"{rows['k_mdct_edge_rows_capped']} v_pk_mul_f32 / v_pk_add_f32, with half of "
                                               f"k_mdct_fwd_small_rows' chain it is {half} (at least {ROWS_LOOP_MACS // 2} each)"))
    capped = [v for k, v in meta.items() if "k_mdct_edge_rows_capped" in k]
    if not capped:
        bad.append(("k_mdct_edge_rows_capped", "no metadata found"))
    for v in capped:
        if v.get("vgpr_count", 1 << 30) > EDGE_CAP_VGPRS or v["lds"] > EDGE_CAP_LDS or v.get("vgpr_spill_count", 1):
            bad.append(("k_mdct_edge_rows_capped", f"{v}: over the cap of {EDGE_CAP_VGPRS} VGPRs / {EDGE_CAP_LDS} bytes of LDS, or spilling"))
    if bad:
        for k, l in bad:
            print(f"check_isa: fused op in {k}: {l}")
        return 1
    print(f"check_isa: {len(seen)} kernels clean (no fused multiply-add)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
