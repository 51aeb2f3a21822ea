"""APC call selection on the device (pw_apc_calls_from_states) against two yardsticks from the same run: a `copy_` of the
state table's bytes, and a `torch.sort` of as many 64-bit words as there are positions. A new capability has no parent figure. One
process, the measurements alternating after a warm-up, host clock around calls that synchronise themselves; per-stage times from the
library's HIP events. Prints one JSON object and writes it to --out.

Workloads over two-instruction blocks, at 2^20 and 2^24 positions:
  spread             a random walk over 2^12 blocks, one basic-block APC per block (its pc constraint): components of one
  hot, no overlap    one block looping, APC A (the block): components of one
  hot, one component the same loop with A and AA (two iterations, higher priority): every candidate in ONE component, the long path

  python tools/bench_apc_calls.py [--log-positions 20 24] [--steps 3] [--warmup 1] [--out profiles/apc_calls.json]"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

LOG_BLOCKS, STRIDE, P = 12, 16, 0x100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-positions", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--second-route-log-positions", type=int, default=20)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "apc_calls.json"))
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_apc_calls: needs a GPU")
    from powdr_amd import abi, stage
    from powdr_amd import apc_calls as ac
    from tests import _apc_calls_ref as ref

    note = lambda *a: print("[bench_apc_calls]", *a, file=sys.stderr, flush=True)
    loop_a = ac.Apc(P, 2, 1, [(ac.Pc(0), ac.Number(P))])
    loop_aa = ac.Apc(P, 4, 2, ac.superblock_pc_constraints([(0, P), (2, P)]))
    block_apcs = [ac.Apc(STRIDE * b, 2, 1, [(ac.Pc(0), ac.Number(STRIDE * b))]) for b in range(1 << LOG_BLOCKS)]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ts):
        return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), ms_all=[round(t, 3) for t in ts])

    def states_of(kind, log_positions):
        """the pcs of 2^log_positions instructions and the state after them"""
        n = 1 << log_positions
        k = torch.arange(n + 1, device="cuda", dtype=torch.int64) % 2
        if kind == "spread":
            g = torch.Generator(device="cuda").manual_seed(log_positions)
            heads = torch.randint(0, 1 << LOG_BLOCKS, (n // 2 + 1,), generator=g, device="cuda", dtype=torch.int64)
            return (STRIDE * torch.repeat_interleave(heads, 2)[:n + 1] + 4 * k).to(torch.int32).contiguous()
        return (P + 4 * k).to(torch.int32).contiguous()

    def measure(name, kind, apcs, log_positions):
        pcs = states_of(kind, log_positions)
        n_states = len(pcs)
        tabs = ac.tables(apcs)
        words = torch.randint(-(1 << 62), 1 << 62, (n_states - 1,), device="cuda", dtype=torch.int64)
        dst = torch.empty_like(pcs)

        def select():
            rc, status, info, handle = stage.raw(ac.lib.pw_apc_calls_from_states, pcs.data_ptr(), None, n_states, 0, 8, *tabs, 0)
            assert (rc, status) == (0, 0) and handle, (rc, status, info)
            with ac.ApcCalls(handle) as got:
                return dict(calls=len(got.calls), covered=got.covered, first_calls=[tuple(c) for c in got.calls[:3]],
                            totals={k: sum(c[k] for c in got.counters) for k in ac.COUNTERS})

        def select_raw():  # the C call and its sizes alone: what a Rust caller pays
            rc, status, info, handle = stage.raw(ac.lib.pw_apc_calls_from_states, pcs.data_ptr(), None, n_states, 0, 8, *tabs, 0)
            assert (rc, status) == (0, 0) and handle, (rc, status, info)
            ac.lib.pw_apc_calls_destroy(handle)

        runs = {"select": select_raw, "copy": lambda: dst.copy_(pcs), "sort": lambda: torch.sort(words)}
        times = {k: [] for k in runs}
        for it in range(args.warmup + args.steps):
            for k in (list(runs) if it % 2 == 0 else list(runs)[::-1]):
                dt, _ = timed(runs[k])
                if it >= args.warmup:
                    times[k].append(dt)
                note(name, it, k, round(dt, 2), "ms")
        run_stats = ac.last_stats()
        abi.lib.powdr_gpu_timing_enable(1)
        result = select()
        torch.cuda.synchronize()
        stages = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in abi.timing_report().items() if k.startswith("apc_calls_")}
        abi.lib.powdr_gpu_timing_enable(0)
        ratio = lambda a, b: dict(median=round(statistics.median(times[a]) / statistics.median(times[b]), 2), min=round(min(times[a]) / max(times[b]), 2),
                                  max=round(max(times[a]) / min(times[b]), 2))
        out = dict(positions=n_states - 1, apcs=len(apcs), state_table_bytes=n_states * 4, runs={k: stats(v) for k, v in times.items()},
                   ns_per_position_median=round(statistics.median(times["select"]) * 1e6 / (n_states - 1), 2), select_over_copy=ratio("select", "copy"),
                   select_over_sort=ratio("select", "sort"), stages_event_timed=stages, result=result, **run_stats)
        long_ms = stages.get("apc_calls_fold_long", {}).get("ms")
        if long_ms is not None and run_stats["long_components"]:
            out["long_path_ns_per_candidate"] = round(long_ms * 1e6 / run_stats["longest_component"], 2)
        return out

    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, workloads={})
    for lp in args.log_positions:
        for name, kind, apcs in (("spread", "spread", block_apcs), ("hot, no overlap", "hot", [loop_a]), ("hot, one component", "hot", [loop_a, loop_aa])):
            key = f"{name} 2^{lp}"
            result["workloads"][key] = measure(key, kind, apcs, lp)
            torch.cuda.empty_cache()
    if args.second_route_log_positions:
        lp = args.second_route_log_positions
        pcs = states_of("hot", lp).tolist()
        tuples = [(P, 2, 1, [(("pc", 0), ("num", P))]), (P, 4, 2, [(("pc", 0), ("num", P)), (("pc", 2), ("num", P))])]
        t0 = time.perf_counter()
        want = ref.select(pcs, tuples)
        result["second_route_hot_one_component"] = dict(positions=1 << lp, wall_s=round(time.perf_counter() - t0, 2), calls=len(want["calls"]))
    result["not_measured"] = ["the trace route at this size (its index stage is §5p's, measured there)", "executions with registers and register-limb constraints",
                              "APCs with thousands of constraints at this size", "a scratch bound below the default",
                              "several long components at once (the long path runs one wave per component)", "the reference's own host loop"]
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
