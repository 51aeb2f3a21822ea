"""The bus half of the mock prover (pw_check_segment_buses) on the C4 HonestSegment, against the only other way to
learn whether the lookup buses balance — HonestSegment.balance_witness(): a second set of provers, a whole segment proof, its
verification. One process, the measurements alternating after a warm-up; the host clock stops after a device synchronise (both calls
synchronise themselves). Prints one JSON object:
  (a) ms of pass A alone (lookup buses; all buses with a table too small to tally) and ms of balance_witness()
  (b) pass A against the summed LogUp permutation kernels of a normal proof of the same AIRs (HIP-event timing of the library)
  (c) pass B: ms, table occupancy and atomics per second with one tampered cell and with tally_all on the lookup buses (the tables
      start at 2^16 slots and are quadrupled while a bus overflows them: `tables` counts every table tallied into)
  (d) the peak scratch bytes of both passes

  python tools/bench_bus_check.py [--max-log-height 20] [--steps 5] [--warmup 2] [--out profiles/bus_check.json]"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-log-height", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--pow-bits", type=int, default=16)
    ap.add_argument("--witness-steps", type=int, default=2, help="timed balance_witness() calls (each proves the segment again)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_bus_check: needs a GPU")
    from oracle import apc_model as om
    from powdr_amd import abi, prover, segment_workload as sw

    seg = sw.HonestSegment("C4", max_log_height=args.max_log_height, seed=0, queries=args.queries, pow_bits=args.pow_bits, logup=True,
                           specialise_all=True)
    seg.generate_traces()
    torch.cuda.synchronize()
    note = lambda *a: print("[bench_bus_check]", *a, file=sys.stderr, flush=True)
    note("segment ready:", len(seg.airs), "AIRs, heights", seg.heights())

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ts):
        return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), ms_all=[round(t, 3) for t in ts])

    runs = {
        "pass_a_lookup_buses": lambda: seg.check_buses(),                              # balanced: pass A is all that runs
        "pass_a_all_buses": lambda: seg.check_buses(None, table_bytes=1, tuple_cap=0),  # no room for one slot: pass A alone
        "tally_all_lookup_buses": lambda: seg.check_buses(tally_all=True),
        "all_buses_default": lambda: seg.check_buses(None, tuple_cap=0),  # the send-only buses are tallied (millions of tuples), not listed
    }
    times = {k: [] for k in runs}
    results, peaks, table_stats = {}, {}, {}
    for it in range(args.warmup + args.steps):
        order = list(runs) if it % 2 == 0 else list(runs)[::-1]
        for k in order:
            dt, results[k] = timed(runs[k])
            peaks[k], table_stats[k] = prover.bus_check_peak_bytes(), prover.bus_check_last_stats()
            if it >= args.warmup:
                times[k].append(dt)
            note(it, k, round(dt, 2), "ms")
    assert all(s["status"] == 0 for s in results["pass_a_lookup_buses"][0]), results["pass_a_lookup_buses"][0]
    assert results["tally_all_lookup_buses"] == results["pass_a_lookup_buses"]

    # (c) one tampered cell: the first cell of the first APC AIR's first var-range argument that is a plain column
    apc = next(a for a in seg.airs if a["role"] == "apc")
    inter, spans, bc = (np.asarray(x) for x in apc["inter"])
    col = None
    for bus, n_args, first in inter.reshape(-1, 3).tolist():
        off, ln = spans.reshape(-1, 2)[first + 1] if n_args else (0, 0)
        if bus == 3 and ln == 2 and bc[off] == 0:
            col = int(bc[off + 1])
            break
    tamper = {}
    if col is not None:
        cell = apc["trace"][col << apc["log_h"]:(col << apc["log_h"]) + 1]
        old = cell.clone()
        v = int(om.from_monty(old.cpu().numpy().view(np.uint32))[0])
        cell.copy_(torch.from_numpy(om.to_monty(np.array([(v + (1 << 24)) % om.P], np.uint32)).view(np.int32)).cuda())
        ts = []
        for it in range(args.warmup + args.steps):
            dt, res = timed(lambda: seg.check_buses())
            if it >= args.warmup:
                ts.append(dt)
        note("tampered cell:", res[0], res[1])
        tamper = dict(stats(ts), summaries=res[0], tuples=res[1], peak_scratch_bytes=prover.bus_check_peak_bytes(), table=prover.bus_check_last_stats())
        # where the time of one such call goes: the library's HIP events around its launches and table clears, and the host clock around it
        abi.lib.powdr_gpu_timing_enable(1)
        dt, _ = timed(lambda: seg.check_buses())
        tamper["one_call_event_timed"] = dict(wall_ms=round(dt, 3), kernels={k: dict(launches=v[0], ms=round(v[1], 3))
                                                                            for k, v in abi.timing_report().items() if k.startswith("bus_")})
        abi.lib.powdr_gpu_timing_enable(0)
        cell.copy_(old)
        torch.cuda.synchronize()

    # (a) the parent's route to the same bit
    witness = []
    for it in range(1 + args.witness_steps):
        dt, (rc, _) = timed(seg.balance_witness)
        note("balance_witness", round(dt, 1), "ms rc", rc)
        assert rc == 0
        if it >= 1:
            witness.append(dt)

    # (b) the LogUp permutation kernels of a normal proof of the same AIRs (HIP events around the launches)
    seg.prove(copy=False)
    abi.lib.powdr_gpu_timing_enable(1)
    seg.prove(copy=False)
    torch.cuda.synchronize()
    report = abi.timing_report()
    abi.lib.powdr_gpu_timing_enable(0)
    perm = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in report.items() if k.startswith("logup_perm")}
    abi.lib.powdr_gpu_timing_enable(1)
    seg.check_buses(None, table_bytes=1, tuple_cap=0)
    seg.check_buses(tally_all=True)
    torch.cuda.synchronize()
    kern = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in abi.timing_report().items() if k.startswith("bus_")}
    abi.lib.powdr_gpu_timing_enable(0)

    out = dict(kind="C4", max_log_height=args.max_log_height, steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
               airs=len(seg.airs), main_cells=seg.cells, heights=seg.heights(),
               logup_paths=sorted({a["prover"].logup_path() for a in seg.airs}),
               summaries_all_buses=results["all_buses_default"][0],
               runs={k: dict(stats(times[k]), peak_scratch_bytes=peaks[k], table=table_stats[k]) for k in runs},
               one_tampered_cell=tamper, balance_witness=stats(witness),
               logup_perm_kernels_of_one_proof=perm, bus_kernels_event_timed=kern)
    a_ms, w_ms = out["runs"]["pass_a_lookup_buses"]["ms_median"], out["balance_witness"]["ms_median"]
    out["pass_a_vs_balance_witness"] = dict(pass_a_ms=a_ms, balance_witness_ms=w_ms, ratio=round(w_ms / a_ms, 2), pass_a_is_faster=a_ms < w_ms)
    perm_ms = sum(v["ms"] for v in perm.values())
    if perm_ms and "bus_sum_kernel" in kern:
        # two event-timed calls above: the first is pass A over all buses, the second pass A over the lookup buses (+ their tally)
        out["pass_a_vs_logup_perm"] = dict(bus_sum_kernel_ms_two_calls=kern["bus_sum_kernel"]["ms"], logup_perm_ms=round(perm_ms, 3),
                                           pass_a_all_buses_wall_ms=out["runs"]["pass_a_all_buses"]["ms_median"],
                                           ratio_wall_over_perm=round(out["runs"]["pass_a_all_buses"]["ms_median"] / perm_ms, 3))
    tall = out["runs"]["tally_all_lookup_buses"]
    b_ms = tall["ms_median"] - a_ms
    if b_ms > 0:
        # per inserted triple: up to two compare-and-swaps on a first visit, then an add, a min and an add
        out["pass_b_tally_all"] = dict(ms=round(b_ms, 3), inserted=tall["table"]["inserted"],
                                       occupancy=round(tall["table"]["occupied_slots"] / max(1, tall["table"]["table_slots"]), 4),
                                       atomics_per_second=round(3 * tall["table"]["inserted"] / (b_ms * 1e-3)))
    print(json.dumps(out))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    seg.close()


if __name__ == "__main__":
    main()
