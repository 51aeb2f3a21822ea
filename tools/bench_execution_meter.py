"""The metered cut of an execution (pw_execution_segments_from_traces_metered) against two yardsticks from the same run:
the unmetered cut on the same traces (everything the meter adds is the difference) and `pw_memory_boundary_trace` over the same rows (one
insert into an address table per access, where the meter inserts up to tree_height + 1 nodes). A new capability has no parent figure
and nothing is gated on a time. §5v's method: one process, the measurements alternating after a warm-up, host clock around calls that
synchronise themselves; per-stage times from the library's HIP events in one further call. Prints one JSON object and writes it to --out.

Workloads: §5v's synthetic state log (every row active, row r is position r; 3 access slots: 41 columns), built on the device, with
honest (as, ptr) columns: `registers` — every access cycles through 8 registers, so the class cap binds and the system counts stay at
8 blocks; `stream` — the first slot of position r touches the fresh block 4 r, the others registers, so a system cap binds.

  python tools/bench_execution_meter.py [--log-positions 20 24] [--log-cap 16] [--steps 3] [--warmup 1] [--out profiles/execution_meter.json]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

TS0, P, N_ACCESS, REGISTERS = 1000, 0x78000001, 3, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-positions", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--log-cap", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "execution_meter.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_execution_meter: needs a GPU")
    from powdr_amd import abi, prover, stage
    from powdr_amd import execution_segments as xs
    from powdr_amd import system_airs as sa
    from tests import _execution_states_ref as sref

    note = lambda *a: print("[bench_execution_meter]", *a, file=sys.stderr, flush=True)
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

    def trace_of(log_positions, stream):
        """the state log of 2^log_positions active rows in time order, column-major, Montgomery: every slot enabled, address space 1,
        data words and previous timestamps 0 (the cut reads neither)"""
        h = 1 << log_positions
        order = torch.arange(h, device="cuda")
        ts = TS0 + N_ACCESS * order
        trace = torch.zeros((width, h), dtype=torch.int32, device="cuda")
        monty = lambda v: ((v.to(torch.int64) << 32) % P).to(torch.int32)
        one = monty(torch.ones_like(ts))
        trace[0], trace[1], trace[2], trace[3], trace[4] = one, monty(4 * (order % 5)), monty(ts), monty(4 * ((order + 1) % 5)), monty(ts + N_ACCESS)
        for j in range(N_ACCESS):
            c = sref.HEAD + sref.PER_ACCESS * j
            trace[c], trace[c + 1] = one, one
            trace[c + 2] = monty(4 * order if stream and j == 0 else 4 * ((order + j) % REGISTERS))
        return trace.reshape(-1)

    def measure(name, trace, pr, log_positions, log_cap):
        n = 1 << log_positions
        seg = [(pr, trace.data_ptr(), log_positions)]
        recs, _ = stage.air_records(seg)
        limits = xs.PwSegmentLimits(log_cap, 0, 0, 0)
        meter = xs.SystemMeter(30, log_cap).record(log_cap)
        none = (None, None, 0, None, None, None, 0)

        def raw_cut(metered):
            if metered:
                rc, status, info, handle = stage.raw(xs.lib.pw_execution_segments_from_traces_metered, recs, None, 1, 0, 0, *none, C.byref(limits), C.byref(meter), 0)
            else:
                rc, status, info, handle = stage.raw(xs.lib.pw_execution_segments_from_traces, recs, None, 1, 0, 0, *none, C.byref(limits), 0)
            assert (rc, status) == (0, 0) and handle, (rc, status, info)
            return handle

        cut = lambda metered: xs.lib.pw_execution_segments_destroy(raw_cut(metered))
        boundary_out = torch.empty(sa.BOUNDARY_WIDTH << (log_positions + 1), dtype=torch.int32, device="cuda")
        boundary = lambda: sa.memory_boundary_trace(seg, log_positions + 1, out=boundary_out)
        got = xs.ExecutionSegments(raw_cut(True), seg, [])
        cut_stats, meter_stats = xs.last_stats(), xs.last_meter_stats()
        plain = xs.ExecutionSegments(raw_cut(False), seg, [])
        _, _, locations, boundary_status = boundary()
        runs = {"metered_cut": lambda: cut(True), "unmetered_cut": lambda: cut(False), "memory_boundary_trace": boundary}
        times = {k: [] for k in runs}
        for step in range(args.warmup + args.steps):
            for k in (list(runs) if step % 2 == 0 else list(runs)[::-1]):
                dt, _ = timed(runs[k])
                if step >= args.warmup:
                    times[k].append(dt)
                note(name, step, k, round(dt, 2), "ms")
        abi.lib.powdr_gpu_timing_enable(1)
        cut(True)
        torch.cuda.synchronize()
        stages = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in abi.timing_report().items() if k.startswith(("execution_segments_", "execution_meter_"))}
        abi.lib.powdr_gpu_timing_enable(0)
        med = lambda k: statistics.median(times[k])
        sys_max = [max((h[k] for h in got.system_heights), default=0) for k in range(3)]
        out = dict(positions=n, width=width, log_cap=log_cap, tree_height=30, trace_bytes=width * n * 4, segments=got.n_segments, unmetered_segments=plain.n_segments,
                   largest_system_heights=dict(boundary=sys_max[0], merkle=sys_max[1], poseidon2_bound=sys_max[2]), first_heights={str(k): v for k, v in got.heights[0].items()},
                   boundary_locations=locations, boundary_status=boundary_status, runs={k: stats(v) for k, v in times.items()}, stages_event_timed=stages,
                   meter_stages_ms=round(sum(v["ms"] for k, v in stages.items() if k.startswith("execution_meter_") and k != "execution_meter_cuts"), 3),
                   metered_over_unmetered_host_clock=round(med("metered_cut") / med("unmetered_cut"), 2),
                   metered_over_boundary_trace_host_clock=round(med("metered_cut") / med("memory_boundary_trace"), 2), last_stats=cut_stats, meter_stats=meter_stats,
                   synchronisations_per_segment=round(meter_stats["synchronisations"] / max(got.n_segments, 1), 2))
        got.close()
        plain.close()
        return out

    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, registers=REGISTERS, workloads={})
    for lp in args.log_positions:
        for stream in (False, True):
            trace = trace_of(lp, stream)
            pr = prover.Prover(width, *no_cons, num_queries=2, interactions=sref.state_log_interactions(N_ACCESS))
            key = f"2^{lp} positions, cap 2^{args.log_cap}, {'stream of fresh blocks' if stream else 'registers'}"
            result["workloads"][key] = measure(key, trace, pr, lp, args.log_cap)
            pr.close()
            del trace
            torch.cuda.empty_cache()
    result["not_measured"] = ["rows permuted against time", "calls (the classes change, the accesses do not)", "a cell budget that binds (probes are counted, not timed)",
                              "a tile other than the default", "tree heights below 30", "the instruction AIRs of a real execution", "hardware counters"]
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
