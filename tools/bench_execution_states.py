"""Register states from traces on the device (pw_execution_states_from_traces) against three yardsticks from the same run:
the existing pcs-only `pw_apc_calls_from_traces` on the same traces, a `copy_` of the register table's bytes, and a `torch.sort` of as
many 64-bit words as there are register sends. A new capability has no parent figure. One process, the measurements alternating after
a warm-up, host clock around calls that synchronise themselves; per-stage times from the library's HIP events in one further call.
Prints one JSON object and writes it to --out.

Workloads: a synthetic state log (tests/_execution_states_ref.py's AIR, built on the device) whose every row is active and makes 3
register accesses, at 2^20 and 2^24 positions:
  spread, 4 / 32 registers   accesses to 32 registers at random, 4 or 32 of them requested
  one register               every access goes to one register: every send lands in one row of the table
The receives carry a previous timestamp shortly before the row's own, as a chained execution's do; the words are not chained (the
routine does not read the chain).

  python tools/bench_execution_states.py [--log-positions 20 24] [--steps 3] [--warmup 1] [--out profiles/execution_states.json]"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

N_ACCESS, TS0, P = 3, 1000, 0x78000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-positions", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "execution_states.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_execution_states: needs a GPU")
    from powdr_amd import abi, prover, stage
    from powdr_amd import apc_calls as ac
    from powdr_amd import execution_states as es
    from tests import _execution_states_ref as sref

    note = lambda *a: print("[bench_execution_states]", *a, file=sys.stderr, flush=True)
    it = sref.state_log_interactions(N_ACCESS)
    width = sref.HEAD + sref.PER_ACCESS * N_ACCESS
    no_cons = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ts):
        return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), ms_all=[round(t, 3) for t in ts])

    def trace_of(log_positions, hot):
        """the state log of 2^log_positions active rows in a random row order, column-major, Montgomery"""
        h = 1 << log_positions
        g = torch.Generator(device="cuda").manual_seed(log_positions)
        rnd = lambda hi, n=h: torch.randint(0, hi, (n,), generator=g, device="cuda", dtype=torch.int64)
        order = torch.randperm(h, generator=g, device="cuda")
        ts = TS0 + N_ACCESS * order
        cols = torch.zeros((width, h), dtype=torch.int64, device="cuda")
        cols[0], cols[1], cols[2], cols[3], cols[4] = 1, 4 * rnd(5), ts, 4 * rnd(5), ts + N_ACCESS
        for j in range(N_ACCESS):
            c = sref.HEAD + sref.PER_ACCESS * j
            cols[c], cols[c + 1], cols[c + 2] = 1, 1, 4 * (torch.full((h,), 5, device="cuda", dtype=torch.int64) if hot else rnd(32))
            for k in range(4):
                cols[c + 3 + k], cols[c + 8 + k] = rnd(256), rnd(256)
            cols[c + 7] = torch.clamp(ts - 1 - rnd(64), min=0)
        return ((cols << 32) % P).to(torch.int32).contiguous().reshape(-1)

    def measure(name, log_positions, hot, regs):
        trace = trace_of(log_positions, hot)
        n = 1 << log_positions
        pr = prover.Prover(width, *no_cons, num_queries=2, interactions=it)
        seg = [(pr, trace.data_ptr(), log_positions)]
        recs, _ = stage.air_records(seg)
        t_regs = (es.C.c_uint32 * len(regs))(*regs)
        tabs = ac.tables([ac.Apc(0, 2, 1, [(ac.Pc(0), ac.Number(0))])])
        table_words = len(regs) * (n + 1)
        src = torch.zeros(table_words, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(src)
        sends = {}

        def states():
            rc, status, info, handle = stage.raw(es.lib.pw_execution_states_from_traces, recs, None, 1, 0, 1, 0, 1, 4, t_regs, len(regs), None, 0)
            assert (rc, status) == (0, 0) and handle, (rc, status, info)
            with es.ExecutionStates(handle) as got:
                sends["n"], sends["states"], sends["bytes"] = got.sends, got.n_states, got.bytes

        def pcs_only():
            rc, status, info, handle = stage.raw(ac.lib.pw_apc_calls_from_traces, recs, None, 1, 0, 0, *tabs, 0)
            assert (rc, status) == (0, 0) and handle, (rc, status, info)
            ac.lib.pw_apc_calls_destroy(handle)

        states()
        words = torch.randint(-(1 << 62), 1 << 62, (max(sends["n"], 1),), device="cuda", dtype=torch.int64)
        runs = {"states": states, "pcs_only_apc_calls": pcs_only, "copy": lambda: dst.copy_(src), "sort": lambda: torch.sort(words)}
        times = {k: [] for k in runs}
        for step in range(args.warmup + args.steps):
            for k in (list(runs) if step % 2 == 0 else list(runs)[::-1]):
                dt, _ = timed(runs[k])
                if step >= args.warmup:
                    times[k].append(dt)
                note(name, step, k, round(dt, 2), "ms")
        run_stats = es.last_stats()
        abi.lib.powdr_gpu_timing_enable(1)
        states()
        torch.cuda.synchronize()
        stages = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in abi.timing_report().items() if k.startswith("execution_states_")}
        abi.lib.powdr_gpu_timing_enable(0)
        pr.close()
        ratio = lambda a, b: round(statistics.median(times[a]) / statistics.median(times[b]), 2)
        return dict(positions=n, registers=len(regs), register_sends=sends["n"], table_bytes=table_words * 4, handle_bytes=sends["bytes"],
                    runs={k: stats(v) for k, v in times.items()}, ns_per_position_median=round(statistics.median(times["states"]) * 1e6 / n, 2),
                    states_over_pcs_only=ratio("states", "pcs_only_apc_calls"), states_over_copy=ratio("states", "copy"), states_over_sort=ratio("states", "sort"),
                    stages_event_timed=stages, stages_ms_total=round(sum(v["ms"] for v in stages.values()), 3), **run_stats)

    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, accesses_per_row=N_ACCESS, fill="LDS tiles", workloads={})
    for lp in args.log_positions:
        for name, hot, regs in (("spread, 4 registers", False, [3, 9, 17, 30]), ("spread, 32 registers", False, list(range(32))), ("one register", True, [5])):
            key = f"{name} 2^{lp}"
            result["workloads"][key] = measure(key, lp, hot, regs)
            torch.cuda.empty_cache()
    result["not_measured"] = ["the instruction AIRs of a real execution at this size (their interaction programs are longer than the state log's)",
                              "the marks-and-scan form of the fill (not built)", "a scratch bound below the default", "the walk's atomics with counters",
                              "pw_apc_calls_from_traces_registers end to end (its selection is §5r's, measured there)", "several segments in flight at once"]
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
