"""Direct mode of applying APC calls (pw_apc_sources_from_traces_flags + pw_apc_sources_tracegen) against two yardsticks
from the same run: (a) the two-step path of the flags-0 interface — `apply_calls`, then `powdr_apc_tracegen_host_tables` on the handle's
source matrices, the same cells — as a whole and as gather + trace generation alone; (b) a `copy_` of the bytes the direct kernel writes.
The method of tools/bench_apc_sources.py: one process, the measurements alternating after a warm-up, host clock around calls that
synchronise themselves, the gather stage from the library's HIP events in one further call. Run it under a `timeout`. Prints one JSON
object and writes it to --out.

Workloads (§5t's): the synthetic state log of tests/_execution_states_ref.py (every row active; 3 accesses: 41 columns), built on the
device, one APC of 8 instructions called at every 16th position; time order (row r is position r) and random order. Cells kept: a
seeded share of the APC's 8 x 41 cells, one APC column each; the output has as many rows as there are calls.

  python tools/bench_apc_direct.py [--log-positions 20 24] [--shares 100 25 5] [--steps 3] [--warmup 1] [--out profiles/apc_direct.json]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

TS0, P, CYCLE, PERIOD = 1000, 0x78000001, 8, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-positions", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--shares", type=int, nargs="+", default=[100, 25, 5])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "apc_direct.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_apc_direct: needs a GPU")
    from powdr_amd import abi, prover, stage
    from powdr_amd import apc_sources as aps
    from tests import _execution_states_ref as sref

    note = lambda *a: print("[bench_apc_direct]", *a, file=sys.stderr, flush=True)
    no_cons = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))
    host_tables = abi.lib.powdr_apc_tracegen_host_tables
    host_tables.restype = C.c_int
    host_tables.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ts):
        return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), ms_all=[round(t, 3) for t in ts])

    def trace_of(log_positions, n_access, random_order):
        """the state log of 2^log_positions active rows, column-major, Montgomery: row r is position r, or position order[r]"""
        h = 1 << log_positions
        width = sref.HEAD + sref.PER_ACCESS * n_access
        g = torch.Generator(device="cuda").manual_seed(log_positions)
        order = torch.randperm(h, generator=g, device="cuda") if random_order else torch.arange(h, device="cuda")
        ts = TS0 + n_access * order
        trace = torch.empty((width, h), dtype=torch.int32, device="cuda")
        monty = lambda v: ((v.to(torch.int64) << 32) % P).to(torch.int32)
        trace[0], trace[1], trace[2], trace[3], trace[4] = monty(torch.ones_like(ts)), monty(4 * (order % 5)), monty(ts), monty(4 * ((order + 1) % 5)), monty(ts + n_access)
        for c in range(sref.HEAD, width):  # the accesses are not read by this routine: any field elements
            trace[c] = torch.randint(0, P, (h,), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
        return trace.reshape(-1), width

    def gather_ms(fn):
        abi.lib.powdr_gpu_timing_enable(1)
        fn()
        torch.cuda.synchronize()
        report = {k: round(v[1], 3) for k, v in abi.timing_report().items() if k.startswith("apc_sources_")}
        abi.lib.powdr_gpu_timing_enable(0)
        return report

    def measure(name, log_positions, random_order):
        trace, width = trace_of(log_positions, 3, random_order)
        n = 1 << log_positions
        pr = prover.Prover(width, *no_cons, num_queries=2, interactions=sref.state_log_interactions(3))
        recs, _ = stage.air_records([(pr, trace.data_ptr(), log_positions)])
        n_calls = n // PERIOD
        start = np.arange(n_calls, dtype=np.uint64) * PERIOD
        end, ids, cycles = start + CYCLE, np.zeros(n_calls, np.uint32), (C.c_uint32 * 1)(CYCLE)
        u32p, u64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)), lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
        every = [(k, c) for k in range(CYCLE) for c in range(width)]
        out = torch.empty(len(every) * n_calls, dtype=torch.int32, device="cuda")
        theirs = torch.empty_like(out)

        def handle(direct):
            rc, status, info, h = stage.raw(aps.lib.pw_apc_sources_from_traces_flags, recs, None, 1, 0, cycles, 1, u32p(ids), u64p(start), u64p(end), n_calls, 0, 0,
                                            aps.DIRECT if direct else 0)
            assert (rc, status) == (0, 0) and h, (rc, status, info)
            return aps.ApcSources(h, [width], direct=direct)

        result = dict(positions=n, width=width, calls=n_calls, trace_bytes=width * n * 4, shares={})
        with handle(True) as d, handle(False) as p:
            result.update(handle_bytes_direct=d.index_bytes + d.residual_bytes, handle_bytes_two_step=p.source_bytes + p.residual_bytes, index_bytes=d.index_bytes,
                          source_bytes=p.source_bytes, residual_bytes=p.residual_bytes)
        for share in args.shares:
            rng = np.random.default_rng([share, log_positions])
            kept = sorted(rng.permutation(len(every))[:max(1, round(len(every) * share / 100))].tolist())
            cells = [(every[i][0], every[i][1], c) for c, i in enumerate(kept)]
            w, written = len(cells), len(cells) * n_calls * 4
            seen = {}

            def direct_tracegen(h):
                h.apc_traces([(0, cells, out.data_ptr(), n_calls, w)])

            def two_step_tracegen(h):
                subs = np.ascontiguousarray(h.substs(0, cells), dtype=np.int32)
                assert host_tables(theirs.data_ptr(), n_calls, None, h.original_airs(0), 1, subs.ctypes.data, len(subs), n_calls) == 0

            def direct_whole():
                with handle(True) as h:
                    seen["direct_peak_bytes"] = aps.last_stats()["peak_bytes"]
                    direct_tracegen(h)

            def two_step_whole():
                with handle(False) as h:
                    seen["two_step_peak_bytes"] = aps.last_stats()["peak_bytes"]
                    two_step_tracegen(h)

            src, dst = torch.zeros(written // 4, dtype=torch.int32, device="cuda"), torch.empty(written // 4, dtype=torch.int32, device="cuda")
            with handle(True) as d, handle(False) as p:
                runs = {"direct_whole": direct_whole, "two_step_whole": two_step_whole, "direct_tracegen": lambda: direct_tracegen(d),
                        "two_step_tracegen": lambda: two_step_tracegen(p), "copy": lambda: dst.copy_(src)}
                times = {k: [] for k in runs}
                for step in range(args.warmup + args.steps):
                    for k in (list(runs) if step % 2 == 0 else list(runs)[::-1]):
                        dt, _ = timed(runs[k])
                        if step >= args.warmup:
                            times[k].append(dt)
                        note(name, share, step, k, round(dt, 2), "ms")
                direct_tracegen(d)
                tg = aps.tracegen_last_stats()
                two_step_tracegen(p)
                torch.cuda.synchronize()
                assert bool((out[:w * n_calls] == theirs[:w * n_calls]).all())  # the two paths wrote the same words
            gd, gp = gather_ms(lambda: handle(True).close()), gather_ms(lambda: handle(False).close())
            med = {k: statistics.median(v) for k, v in times.items()}
            alone_d, alone_p = gd["apc_sources_gather"] + med["direct_tracegen"], gp["apc_sources_gather"] + med["two_step_tracegen"]
            result["shares"][f"{share} %"] = dict(
                cells=w, bytes_written=written, runs={k: stats(v) for k, v in times.items()}, gather_ms_direct_handle=gd["apc_sources_gather"],
                gather_ms_two_step_handle=gp["apc_sources_gather"], direct_over_two_step_whole=round(med["direct_whole"] / med["two_step_whole"], 3),
                direct_over_two_step_gather_and_tracegen=round(alone_d / alone_p, 3), direct_tracegen_over_two_step_tracegen=round(med["direct_tracegen"] / med["two_step_tracegen"], 3),
                direct_tracegen_over_copy=round(med["direct_tracegen"] / med["copy"], 2), direct_tracegen_gb_per_s_written=round(written / med["direct_tracegen"] / 1e6, 1),
                tracegen_stats=tg, **seen)
            del src, dst
        pr.close()
        return result

    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, apc_cycle_count=CYCLE, call_period=PERIOD, workloads={})
    todo = [("time order 2^20", 20, False), ("random order 2^20", 20, True), ("time order 2^24", 24, False)]
    for key, lp, rnd in [t for t in todo if t[1] in args.log_positions]:
        result["workloads"][key] = measure(key, lp, rnd)
        torch.cuda.empty_cache()
    result["not_measured"] = ["the instruction AIRs of a real execution (thirteen chips, several APCs, cells chosen by the optimiser and not at random)",
                              "hardware counters (the sectors the strided list and trace reads fetch are the supposed reason for the distance from the copy)",
                              "random order at 2^24 positions", "a scratch bound below the default", "several segments in flight at once"]
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
