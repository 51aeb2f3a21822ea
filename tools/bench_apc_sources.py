"""Applying APC calls on the device (pw_apc_sources_from_traces) against two yardsticks from the same run: a `copy_` of as
many bytes as the call writes (sources + residuals), against which the gather stage alone is compared, and the pcs-only
`pw_apc_calls_from_traces` on the same traces, against which the index and place stages are compared. A new capability has no parent
figure. One process, the measurements alternating after a warm-up, host clock around calls that synchronise themselves; per-stage
times from the library's HIP events in one further call, the copy timed by events as well. Prints one JSON object and writes it to
--out.

Workloads: the synthetic state log of tests/_execution_states_ref.py (every row active; 3 accesses: 41 columns, LoadStore's width),
built on the device, with one APC of 8 instructions called at every 16th position — the calls cover half the positions:
  time order     row r is position r: source and residual index lists are runs of 8 consecutive rows, every load a 16-byte load
  random order   the positions lie at random rows: the sources read single rows all over the trace, the residual's ascending rows have
                 holes at random
  wide           13 accesses: 161 columns, time order, at the smaller size only

  python tools/bench_apc_sources.py [--log-positions 20 24] [--steps 3] [--warmup 1] [--out profiles/apc_sources.json]"""
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
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "apc_sources.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_apc_sources: needs a GPU")
    from powdr_amd import abi, prover, stage
    from powdr_amd import apc_calls as ac
    from powdr_amd import apc_sources as aps
    from tests import _execution_states_ref as sref

    note = lambda *a: print("[bench_apc_sources]", *a, file=sys.stderr, flush=True)
    no_cons = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))

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

    def measure(name, log_positions, n_access, random_order):
        trace, width = trace_of(log_positions, n_access, random_order)
        n = 1 << log_positions
        pr = prover.Prover(width, *no_cons, num_queries=2, interactions=sref.state_log_interactions(n_access))
        recs, _ = stage.air_records([(pr, trace.data_ptr(), log_positions)])
        n_calls = n // PERIOD
        start = np.arange(n_calls, dtype=np.uint64) * PERIOD
        end, ids, cycles = start + CYCLE, np.zeros(n_calls, np.uint32), (C.c_uint32 * 1)(CYCLE)
        u32p, u64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)), lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
        tabs = ac.tables([ac.Apc(0, 2, 1, [(ac.Pc(0), ac.Number(0))])])
        seen = {}

        def apply():
            rc, status, info, handle = stage.raw(aps.lib.pw_apc_sources_from_traces, recs, None, 1, 0, cycles, 1, u32p(ids), u64p(start), u64p(end), n_calls, 0, 0)
            assert (rc, status) == (0, 0) and handle, (rc, status, info)
            with aps.ApcSources(handle, [width]) as got:
                seen.update(written=got.source_bytes + got.residual_bytes, residual_rows=got.residual(0).rows, source_width_height_rbs=tuple(got.source(0, 0))[1:])

        def pcs_only():
            rc, status, info, handle = stage.raw(ac.lib.pw_apc_calls_from_traces, recs, None, 1, 0, 0, *tabs, 0)
            assert (rc, status) == (0, 0) and handle, (rc, status, info)
            ac.lib.pw_apc_calls_destroy(handle)

        apply()
        written = seen["written"]
        src = torch.zeros(written // 4, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(src)
        runs = {"apply": apply, "pcs_only_apc_calls": pcs_only, "copy": lambda: dst.copy_(src)}
        times = {k: [] for k in runs}
        for step in range(args.warmup + args.steps):
            for k in (list(runs) if step % 2 == 0 else list(runs)[::-1]):
                dt, _ = timed(runs[k])
                if step >= args.warmup:
                    times[k].append(dt)
                note(name, step, k, round(dt, 2), "ms")
        run_stats = aps.last_stats()
        copy_events = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            copy_events.append(e0.elapsed_time(e1))
        report = {}
        for what, fn in (("apc_sources_", apply), ("apc_calls_", pcs_only)):
            abi.lib.powdr_gpu_timing_enable(1)
            fn()
            torch.cuda.synchronize()
            report[what] = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in abi.timing_report().items() if k.startswith(what)}
            abi.lib.powdr_gpu_timing_enable(0)
        pr.close()
        stages, theirs = report["apc_sources_"], report["apc_calls_"]
        gather_ms, copy_ms = stages["apc_sources_gather"]["ms"], statistics.median(copy_events)
        index_place = sum(v["ms"] for k, v in stages.items() if k != "apc_sources_gather")
        return dict(positions=n, width=width, calls=n_calls, trace_bytes=width * n * 4, **seen, runs={k: stats(v) for k, v in times.items()},
                    copy_ms_by_events=[round(t, 3) for t in copy_events], stages_event_timed=stages, pcs_only_stages_event_timed=theirs,
                    gather_over_copy=round(gather_ms / copy_ms, 2), gather_gb_per_s_written=round(written / gather_ms / 1e6, 1),
                    index_and_place_ms=round(index_place, 3), pcs_only_stages_ms=round(sum(v["ms"] for v in theirs.values()), 3),
                    index_and_place_over_pcs_only=round(index_place / max(sum(v["ms"] for v in theirs.values()), 1e-9), 2),
                    apply_over_pcs_only_host_clock=round(statistics.median(times["apply"]) / statistics.median(times["pcs_only_apc_calls"]), 2), **run_stats)

    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, apc_cycle_count=CYCLE, call_period=PERIOD, workloads={})
    todo = [(f"{name} 2^{lp}", lp, 3, rnd) for lp in args.log_positions for name, rnd in (("time order", False), ("random order", True))]
    todo.append((f"wide, time order 2^{min(args.log_positions)}", min(args.log_positions), 13, False))
    for key, lp, n_access, rnd in todo:
        result["workloads"][key] = measure(key, lp, n_access, rnd)
        torch.cuda.empty_cache()
    result["not_measured"] = ["the instruction AIRs of a real execution at this size (thirteen chips, several APCs: more jobs, the same bytes)",
                              "hardware counters of the random-order gather (sector reads are the supposed reason for its distance from the copy)",
                              "a scratch bound below the default", "several segments in flight at once", "the APC trace generator on the sources (§5a, measured there)"]
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
