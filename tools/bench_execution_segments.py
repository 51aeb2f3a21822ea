"""Cutting an execution into segments on the device (pw_execution_segments_from_traces) against two yardsticks from the
same run: the pcs-only `pw_apc_calls_from_traces` with no APC that matches on the same traces — the time index alone — against which the
stages after the time index are compared, and a `copy_` of as many bytes as the gathers of all segments write, against which that
gather (one `pw_trace_gather_rows` call for all segments) is compared. A new capability has no parent figure. §5t's method: one process,
the measurements alternating after a warm-up, host clock around calls that synchronise themselves; per-stage times from the library's
HIP events in one further call. Prints one JSON object and writes it to --out.

Workloads: the synthetic state log of tests/_execution_states_ref.py (every row active, row r is position r; 3 accesses: 41 columns,
LoadStore's width), built on the device; height caps 2^16 and 2^20; without calls, and with one APC of 8 instructions called at every
16th position (the calls cover half the positions, so a segment holds twice the cap in original rows).

  python tools/bench_execution_segments.py [--log-positions 20 24] [--log-caps 16 20] [--steps 3] [--warmup 1] [--out profiles/execution_segments.json]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

TS0, P, CYCLE, PERIOD, N_ACCESS = 1000, 0x78000001, 8, 16, 3
INDEX_STAGES = ("execution_segments_index_kernel", "execution_segments_sort_time", "execution_segments_time_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-positions", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--log-caps", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "execution_segments.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_execution_segments: needs a GPU")
    from powdr_amd import abi, prover, stage
    from powdr_amd import apc_calls as ac
    from powdr_amd import apc_sources as aps
    from powdr_amd import execution_segments as xs
    from tests import _execution_states_ref as sref

    note = lambda *a: print("[bench_execution_segments]", *a, file=sys.stderr, flush=True)
    no_cons = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))
    width = sref.HEAD + sref.PER_ACCESS * N_ACCESS

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ts):
        return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), ms_all=[round(t, 3) for t in ts])

    def trace_of(log_positions):
        """the state log of 2^log_positions active rows in time order, column-major, Montgomery"""
        h = 1 << log_positions
        g = torch.Generator(device="cuda").manual_seed(log_positions)
        order = torch.arange(h, device="cuda")
        ts = TS0 + N_ACCESS * order
        trace = torch.empty((width, h), dtype=torch.int32, device="cuda")
        monty = lambda v: ((v.to(torch.int64) << 32) % P).to(torch.int32)
        trace[0], trace[1], trace[2], trace[3], trace[4] = monty(torch.ones_like(ts)), monty(4 * (order % 5)), monty(ts), monty(4 * ((order + 1) % 5)), monty(ts + N_ACCESS)
        for c in range(sref.HEAD, width):  # the accesses are not read by this routine: any field elements
            trace[c] = torch.randint(0, P, (h,), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
        return trace.reshape(-1)

    def measure(name, trace, pr, log_positions, log_cap, with_calls):
        n = 1 << log_positions
        seg = [(pr, trace.data_ptr(), log_positions)]
        recs, _ = stage.air_records(seg)
        n_calls = n // PERIOD if with_calls else 0
        start = np.arange(max(n_calls, 1), dtype=np.uint64) * PERIOD
        end, ids = start + CYCLE, np.zeros(max(n_calls, 1), np.uint32)
        cycles, widths = (C.c_uint32 * 1)(CYCLE), (C.c_uint32 * 1)(4 * width)
        u32p, u64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)), lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
        limits = xs.PwSegmentLimits(log_cap, 0, 0, 0)
        tabs = ac.tables([ac.Apc(0, 2, 1, [(ac.Pc(0), ac.Number(0))])])

        def raw_cut():
            rc, status, info, handle = stage.raw(xs.lib.pw_execution_segments_from_traces, recs, None, 1, 0, 0, cycles, widths, 1, u32p(ids), u64p(start), u64p(end), n_calls, C.byref(limits), 0)
            assert (rc, status) == (0, 0) and handle, (rc, status, info)
            return handle

        def cut():
            xs.lib.pw_execution_segments_destroy(raw_cut())

        def pcs_only():
            rc, status, info, handle = stage.raw(ac.lib.pw_apc_calls_from_traces, recs, None, 1, 0, 0, *tabs, 0)
            assert (rc, status) == (0, 0) and handle, (rc, status, info)
            ac.lib.pw_apc_calls_destroy(handle)

        got = xs.ExecutionSegments(raw_cut(), seg, [])  # (only `.calls(s)` would read the calls)
        cut_stats = xs.last_stats()
        jobs, outs = [], []
        for s in range(got.n_segments):
            ptr, rows, lh = got.rows(s, 0)
            outs.append(torch.empty(width << lh, dtype=torch.int32, device="cuda"))
            jobs.append(aps.GatherJob(trace.data_ptr(), n, width, ptr, outs[-1].data_ptr(), 1 << lh))
        written = 4 * sum(t.numel() for t in outs)
        src = torch.zeros(written // 4, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(src)
        runs = {"cut": cut, "pcs_only_apc_calls": pcs_only, "gather_all_segments": lambda: aps.gather_rows(jobs), "copy": lambda: dst.copy_(src)}
        times = {k: [] for k in runs}
        for step in range(args.warmup + args.steps):
            for k in (list(runs) if step % 2 == 0 else list(runs)[::-1]):
                dt, _ = timed(runs[k])
                if step >= args.warmup:
                    times[k].append(dt)
                note(name, step, k, round(dt, 2), "ms")
        gather_stats = aps.last_stats()
        report = {}
        for what, fn in (("execution_segments_", cut), ("apc_calls_", pcs_only), ("apc_sources_gather", lambda: aps.gather_rows(jobs))):
            abi.lib.powdr_gpu_timing_enable(1)
            fn()
            torch.cuda.synchronize()
            report[what] = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in abi.timing_report().items() if k.startswith(what)}
            abi.lib.powdr_gpu_timing_enable(0)
        stages, theirs = report["execution_segments_"], report["apc_calls_"]
        after_index = sum(v["ms"] for k, v in stages.items() if k not in INDEX_STAGES)
        index_ms = sum(v["ms"] for k, v in stages.items() if k in INDEX_STAGES)
        med = lambda k: statistics.median(times[k])
        out = dict(positions=n, width=width, log_cap=log_cap, calls=n_calls, trace_bytes=width * n * 4, segments=got.n_segments, list_bytes=got.list_bytes,
                   first_heights={str(k): v for k, v in got.heights[0].items()}, gather_bytes_written=written, runs={k: stats(v) for k, v in times.items()},
                   stages_event_timed=stages, pcs_only_stages_event_timed=theirs, gather_event_timed=report["apc_sources_gather"],
                   stages_after_index_ms=round(after_index, 3), own_index_stages_ms=round(index_ms, 3), pcs_only_stages_ms=round(sum(v["ms"] for v in theirs.values()), 3),
                   stages_after_index_over_time_index=round(after_index / max(index_ms, 1e-9), 3),
                   cut_over_pcs_only_host_clock=round(med("cut") / med("pcs_only_apc_calls"), 2), gather_over_copy_host_clock=round(med("gather_all_segments") / med("copy"), 2),
                   gather_tiles_16_byte_loads=gather_stats["tiles_16_byte_loads"], gather_tiles_4_byte_loads=gather_stats["tiles_4_byte_loads"], last_stats=cut_stats)
        got.close()
        return out

    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, apc_cycle_count=CYCLE, call_period=PERIOD, workloads={})
    for lp in args.log_positions:
        trace = trace_of(lp)
        pr = prover.Prover(width, *no_cons, num_queries=2, interactions=sref.state_log_interactions(N_ACCESS))
        for cap in args.log_caps:
            for with_calls in (False, True):
                key = f"2^{lp} positions, cap 2^{cap}, {'calls at every 16th position' if with_calls else 'no calls'}"
                result["workloads"][key] = measure(key, trace, pr, lp, cap, with_calls)
                torch.cuda.empty_cache()
        pr.close()
        del trace
        torch.cuda.empty_cache()
    result["not_measured"] = ["rows permuted against time (the gather then reads single rows: §5t's random-order figures)",
                              "the instruction AIRs of a real execution (thirteen chips, several APCs: more classes, the same positions)",
                              "a cell budget that binds (the bisection's probes are counted, not timed on their own)",
                              "a cap so small that the one-workgroup loop over the segments dominates",
                              "a scratch bound below the default", "hardware counters"]
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
