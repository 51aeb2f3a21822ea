"""Empirical constraints on the device (pw_empirical_detect) against two yardsticks from the same run: a `copy_` of the
active cells' bytes, which the gather cannot beat, and a `torch.sort` of the same number of 32-bit words, which the exact
percentiles cannot beat by much. A new capability has no parent figure. One process, the measurements alternating after a warm-up,
host clock around calls that synchronise themselves; per-stage times from the library's HIP events. Prints one JSON object and
writes it to --out.

Workload: one block-log AIR (main columns [is_valid, pc, ts, 29 data words]: width 32) built with torch on the device, blocks of 8
instructions; 2^14, 2^17 and 2^20 instances of ONE block (the hot-pc case) and the same rows spread over 2^12 blocks.

  python tools/bench_empirical.py [--log-instances 14 17 20] [--steps 3] [--warmup 1] [--out profiles/empirical_constraints.json]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

WIDTH, INSTRUCTIONS, P = 32, 8, 0x78000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-instances", type=int, nargs="+", default=[14, 17, 20])
    ap.add_argument("--log-blocks", type=int, default=12)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "empirical_constraints.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_empirical: needs a GPU")
    from powdr_amd import abi, empirical, prover, stage
    from tests import _empirical_ref as ref

    note = lambda *a: print("[bench_empirical]", *a, file=sys.stderr, flush=True)
    no_cons = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))
    p = prover.Prover(WIDTH, *no_cons, num_queries=2, interactions=ref.block_log_interactions())

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ts):
        return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), ms_all=[round(t, 3) for t in ts])

    def workload(log_instances, log_blocks):
        """rows in time order: instance j of block (j mod 2^log_blocks), instruction k, at timestamp 1 + 8 j + k; data word d is a
        random word for d < 8, and word (d mod 8) again for the others but the last, so that every block has classes to verify"""
        n = INSTRUCTIONS << log_instances
        g = torch.Generator(device="cuda").manual_seed(log_instances * 64 + log_blocks)
        row = torch.arange(n, device="cuda", dtype=torch.int64)
        inst, k = row // INSTRUCTIONS, row % INSTRUCTIONS
        cols = torch.empty((WIDTH, n), dtype=torch.int64, device="cuda")
        cols[0] = 1
        cols[1] = (inst % (1 << log_blocks)) * 64 + 4 * k
        cols[2] = 1 + row
        cols[3:11] = torch.randint(0, P, (8, n), generator=g, device="cuda", dtype=torch.int64)
        for d in range(8, WIDTH - 4):
            cols[3 + d] = cols[3 + d % 8]
        cols[WIDTH - 1] = torch.randint(0, 256, (n,), generator=g, device="cuda", dtype=torch.int64)
        trace = ((cols << 32) % P).to(torch.int32).contiguous().reshape(-1)  # Montgomery words
        blocks = [(64 * b, INSTRUCTIONS) for b in range(1 << log_blocks)]
        return trace, n, blocks

    def measure(name, log_instances, log_blocks):
        trace, n, blocks = workload(log_instances, log_blocks)
        log_h = n.bit_length() - 1
        recs, _ = stage.air_records([(p, trace.data_ptr(), log_h)])
        blk = (empirical.PwBasicBlock * len(blocks))(*[empirical.PwBasicBlock(s, c) for s, c in blocks])
        words = torch.randint(-(1 << 31), (1 << 31) - 1, (n * WIDTH,), device="cuda", dtype=torch.int32)
        dst = torch.empty_like(trace)

        def detect():
            rc, status, info, handle = stage.raw(empirical.lib.pw_empirical_detect, recs, None, 1, 0, 4, blk, len(blocks), 0)
            assert (rc, status) == (0, 0) and handle, (rc, status, info)
            sizes = (C.c_uint64 * 5)()
            empirical.lib.pw_empirical_sizes(handle, sizes)
            empirical.lib.pw_empirical_destroy(handle)
            return [int(x) for x in sizes]

        runs = {"detect": detect, "copy": lambda: dst.copy_(trace), "sort": lambda: torch.sort(words)}
        times, last = {k: [] for k in runs}, {}
        for it in range(args.warmup + args.steps):
            for k in (list(runs) if it % 2 == 0 else list(runs)[::-1]):
                dt, last[k] = timed(runs[k])
                if it >= args.warmup:
                    times[k].append(dt)
                note(name, it, k, round(dt, 2), "ms")
        run_stats = empirical.last_stats()
        abi.lib.powdr_gpu_timing_enable(1)
        detect()
        torch.cuda.synchronize()
        stages = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in abi.timing_report().items() if k.startswith("empirical_")}
        abi.lib.powdr_gpu_timing_enable(0)
        ratio = lambda a, b: dict(median=round(statistics.median(times[a]) / statistics.median(times[b]), 2), min=round(min(times[a]) / max(times[b]), 2),
                                  max=round(max(times[a]) / min(times[b]), 2))
        pcs, ranges, seen, classes, cells = last["detect"]
        return dict(rows=n, blocks=len(blocks), cell_bytes=n * WIDTH * 4, pcs=pcs, blocks_seen=seen, classes=classes, cells_in_classes=cells,
                    runs={k: stats(v) for k, v in times.items()}, detect_over_copy=ratio("detect", "copy"), detect_over_sort=ratio("detect", "sort"),
                    stages_event_timed=stages, panels=run_stats["panels"], seeds=run_stats["seeds"], cells_verified=run_stats["cells_verified"],
                    peak_scratch_bytes=run_stats["peak_bytes"])

    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, width=WIDTH, instructions=INSTRUCTIONS, hot={}, spread={})
    for li in args.log_instances:
        result["hot"][f"2^{li}"] = measure(f"hot 2^{li}", li, 0)
        if li >= args.log_blocks:
            result["spread"][f"2^{li}"] = measure(f"spread 2^{li}", li, args.log_blocks)
        torch.cuda.empty_cache()
    result["not_measured"] = ["AIRs of different widths in one call (the panel sorts the absent columns' slots too)", "the interpreter path (POWDR_LOGUP_INTERPRET=1)",
                              "a scratch bound that forces several panels", "the instruction chips' own traces at this size"]
    p.close()
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
