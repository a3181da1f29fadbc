#!/usr/bin/env python3
"""Rates of the two distance kernels (biogarden_amd/csrc/bg_dist.hip) on one GPU; prints one JSON
line with two results.

(i)  "matrix": bg_mismatch_matrix of ROWS x COLS DNA against itself (default 4096 x 10 000).
     Kernel time from device events (bg_dist_last_ms; the launch repeated inside one call until
     the timed window is a good fraction of a second), host-to-host wall time of a plain call,
     byte comparisons per second over the N^2 L / 2 comparisons of the upper triangle, and the
     share of the VALU bound.  The bound is lanes x clock x 4 bytes / VALU_PER_WORD, with
     VALU_PER_WORD counted in the kernel's ISA (below).  In the same run, alternating, the tiled
     kernel against the route that needs no matrix kernel: the pair kernel over all N x N pairs
     (BG_DIST_ROUTE=pairs); both results must be identical.
(ii) "pairs": bg_hamming_batch of PAIRS x PAIR_BYTES (default 256 x 4 MiB), two bytes read per
     position, in GB/s against the HBM figures of the MI355X (8.0 TB/s peak, 6.29 TB/s measured
     with a float4 copy).

No GPU, no number: without a device the handle cannot be made and the tool fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# VALU instructions of bg_dist_tile_kernel's slab loop per 4-byte word comparison, counted in the
# ISA hipcc saves for gfx950 (--save-temps, ROCm 7): one unrolled slab is 256 word comparisons
# (16 words x 4 x 4) and holds 256 each of v_xor_b32, v_and_b32, v_add_u32, v_bitop3_b32 and
# v_bcnt_u32_b32 = 1280 VALU instructions, 5 per word (1.25 per byte comparison).  The bound below
# prices every one of them at the guide's 2 cycles per wave64 instruction; the two three-operand
# forms measure about 4.4 (DESIGN.md "Distances"), so the share understates how close the loop is
# to what the SIMD issues.
VALU_PER_WORD = 1280 / 256
LANES = 256 * 4 * 32            # CUs x SIMDs x lanes issuing per clock
CLOCK_HZ = 2.4e9
HBM_PEAK, HBM_MEASURED = 8.0e12, 6.29e12


def dna(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def timed(h, call, window_ms=300.0):
    """Kernel ms per launch: one plain call sizes BG_DIST_REPEAT so that the launches between the
    two events fill window_ms."""
    os.environ.pop("BG_DIST_REPEAT", None)
    out = call()
    one = max(h.dist_last_ms(), 1e-3)
    reps = int(min(max(window_ms / one, 1), 2000))
    os.environ["BG_DIST_REPEAT"] = str(reps)
    try:
        out = call()
        return h.dist_last_ms(), reps, out
    finally:
        os.environ.pop("BG_DIST_REPEAT", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--cols", type=int, default=10000)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--pair-bytes", type=int, default=4 << 20)
    ap.add_argument("--ab", type=int, default=3, help="tiled / pairs alternations")
    args = ap.parse_args()
    from biogarden_amd import _native
    h = _native.Handle(0)
    rng = np.random.default_rng(1)

    # ---- (i) the matrix
    N, L = args.rows, args.cols
    rows = [dna(rng, L) for _ in range(N)]
    for _ in range(2):
        h.mismatch_matrix(rows)                                   # warm-up
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        h.mismatch_matrix(rows)
        walls.append((time.perf_counter() - t0) * 1e3)
    tiled, pairs_route, ref = [], [], None
    for _ in range(args.ab):
        os.environ.pop("BG_DIST_ROUTE", None)
        ms, reps, out = timed(h, lambda: h.mismatch_matrix(rows))
        tiled.append(ms)
        ref = out
        os.environ["BG_DIST_ROUTE"] = "pairs"
        try:
            ms2, reps2, out2 = timed(h, lambda: h.mismatch_matrix(rows))
        finally:
            os.environ.pop("BG_DIST_ROUTE", None)
        pairs_route.append(ms2)
        if not (out == out2).all():
            raise SystemExit("tiled and pair routes disagree")
    sample = [0, N // 3, N - 1]
    for i in sample:
        want = [(np.frombuffer(rows[i], np.uint8) != np.frombuffer(rows[j], np.uint8)).sum() for j in sample]
        if list(ref[i, sample]) != want:
            raise SystemExit("matrix differs from NumPy at row %d" % i)
    comps = N * N * L / 2
    kms = min(tiled)
    rate = comps / (kms * 1e-3)
    bound = LANES * CLOCK_HZ * 4 / VALU_PER_WORD
    matrix = {"rows": N, "cols": L, "kernel_ms": round(kms, 4), "kernel_ms_all": [round(x, 4) for x in tiled],
              "launches_per_window": reps, "wall_ms": round(sorted(walls)[1], 2),
              "byte_comparisons": comps, "byte_comparisons_per_s": rate,
              "valu_per_word": VALU_PER_WORD, "valu_bound_per_s": bound,
              "share_of_valu_bound": round(rate / bound, 4),
              "pairs_route_ms_all": [round(x, 4) for x in pairs_route],
              "tiled_over_pairs_route": round(min(pairs_route) / kms, 2)}
    del rows, ref, out, out2

    # ---- (ii) the pair kernel
    P, B = args.pairs, args.pair_bytes
    bufs = [dna(rng, B) for _ in range(8)]
    pairs = [(bufs[p % 8], bufs[(p + 3) % 8]) for p in range(P)]
    res = {}
    for name, ts in (("mismatches_and_transitions", True), ("mismatches_only", False)):
        h.hamming_batch(pairs[:2], transitions=ts)               # warm-up (code object)
        ms, reps, out = timed(h, lambda: h.hamming_batch(pairs, transitions=ts))
        a, b = np.frombuffer(pairs[1][0], np.uint8), np.frombuffer(pairs[1][1], np.uint8)
        if out[0][1] != int((a != b).sum()) or any(out[2]):
            raise SystemExit("pair counts differ from NumPy")
        bps = 2.0 * P * B / (ms * 1e-3)
        res[name] = {"kernel_ms": round(ms, 4), "launches_per_window": reps, "GB_per_s": round(bps / 1e9, 1),
                     "share_of_hbm_peak_8.0TBs": round(bps / HBM_PEAK, 4),
                     "share_of_hbm_measured_6.29TBs": round(bps / HBM_MEASURED, 4)}
    res.update({"pairs": P, "bytes_per_sequence": B, "bytes_read": 2 * P * B})
    h.close()
    print(json.dumps({"matrix": matrix, "pairs": res}))


if __name__ == "__main__":
    main()
