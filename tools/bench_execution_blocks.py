"""Superblock detection on the device (pw_execution_blocks_from_pcs) against two yardsticks from the same run: a `copy_`
of the pc list, and a `torch.sort` of as many 64-bit words as there are heads — the window naming is max_bb − 1 such sorts and the
counts ride on the same sort, so that is the floor. A new capability has no parent figure. One process, the measurements alternating
after a warm-up, host clock around calls that synchronise themselves; per-stage times from the library's HIP events. Prints one JSON
object and writes it to --out.

Workloads over 2^12 two-instruction blocks and one one-instruction block (the cut), at 2^20 and 2^24 heads, max_bb 1 and 4:
  hot       one run, three blocks repeating (every window of length 4 overlaps itself: one cluster of a million)
  spread    a random walk over the blocks, every eighth head on average a cut: many short runs
  distinct  random runs of 2^12 heads between cuts: every run distinct

  python tools/bench_execution_blocks.py [--log-heads 20 24] [--max-bb 1 4] [--steps 3] [--warmup 1] [--out profiles/execution_blocks.json]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

LOG_BLOCKS, STRIDE = 12, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-heads", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--max-bb", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--second-route-log-heads", type=int, default=20)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "execution_blocks.json"))
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_execution_blocks: needs a GPU")
    from powdr_amd import abi, empirical, stage
    from powdr_amd import execution_blocks as eb
    from tests import _execution_blocks_ref as ref

    note = lambda *a: print("[bench_execution_blocks]", *a, file=sys.stderr, flush=True)
    n_multi = 1 << LOG_BLOCKS
    cut = n_multi  # the index of the one-instruction block
    blocks = [(STRIDE * b, 2) for b in range(n_multi)] + [(STRIDE * cut, 1)]
    blk = (empirical.PwBasicBlock * len(blocks))(*[empirical.PwBasicBlock(s, c) for s, c in blocks])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ts):
        return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), ms_all=[round(t, 3) for t in ts])

    def heads_of(kind, log_heads):
        n = 1 << log_heads
        g = torch.Generator(device="cuda").manual_seed(log_heads * 8 + len(kind))
        i = torch.arange(n, device="cuda", dtype=torch.int64)
        if kind == "hot":
            return 5 + i % 3
        h = torch.randint(0, n_multi, (n,), generator=g, device="cuda", dtype=torch.int64)
        if kind == "spread":
            return torch.where(torch.randint(0, 8, (n,), generator=g, device="cuda") == 0, torch.full_like(h, cut), h)
        return torch.where(i % (1 << 12) == (1 << 12) - 1, torch.full_like(h, cut), h)

    def pcs_of(heads):
        length = torch.where(heads == cut, 1, 2)
        first = torch.cumsum(length, 0) - length
        rep = torch.repeat_interleave(torch.arange(len(heads), device="cuda"), length)
        k = torch.arange(len(rep), device="cuda") - first[rep]
        return (STRIDE * heads[rep] + 4 * k).to(torch.int32).contiguous()

    def measure(name, kind, log_heads, max_bb):
        heads = heads_of(kind, log_heads)
        pcs = pcs_of(heads)
        n_heads, n = len(heads), len(pcs)
        words = torch.randint(-(1 << 62), 1 << 62, (n_heads,), device="cuda", dtype=torch.int64)
        dst = torch.empty_like(pcs)

        def detect(keep=False):
            rc, status, info, handle = stage.raw(eb.lib.pw_execution_blocks_from_pcs, pcs.data_ptr(), n, 4, blk, len(blocks), max_bb, 0)
            assert (rc, status) == (0, 0) and handle, (rc, status, info)
            sizes = (C.c_uint64 * 6)()
            eb.lib.pw_execution_blocks_sizes(handle, sizes)
            if keep:
                return handle
            eb.lib.pw_execution_blocks_destroy(handle)
            return [int(x) for x in sizes]

        runs = {"detect": detect, "copy": lambda: dst.copy_(pcs), "sort": lambda: torch.sort(words)}
        times, last = {k: [] for k in runs}, {}
        for it in range(args.warmup + args.steps):
            for k in (list(runs) if it % 2 == 0 else list(runs)[::-1]):
                dt, last[k] = timed(runs[k])
                if it >= args.warmup:
                    times[k].append(dt)
                note(name, it, k, round(dt, 2), "ms")
        run_stats = eb.last_stats()
        abi.lib.powdr_gpu_timing_enable(1)
        handle = detect(keep=True)
        torch.cuda.synchronize()
        stages = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in abi.timing_report().items() if k.startswith("execution_blocks_")}
        abi.lib.powdr_gpu_timing_enable(0)
        # a candidate re-counted on the resident execution: the first two heads as the needle
        needle = (C.c_uint32 * 2)(*[STRIDE * int(x) for x in heads[:2].tolist()])
        out = C.c_uint64()
        count_ms = []
        for _ in range(args.steps):
            dt, rc = timed(lambda: eb.lib.pw_execution_blocks_count(handle, needle, 2, 0, C.byref(out)))
            assert rc == 0
            count_ms.append(dt)
        eb.lib.pw_execution_blocks_destroy(handle)
        ratio = lambda a, b: dict(median=round(statistics.median(times[a]) / statistics.median(times[b]), 2), min=round(min(times[a]) / max(times[b]), 2),
                                  max=round(max(times[a]) / min(times[b]), 2))
        n_pcs, n_runs, _, n_sb, _, resident = last["detect"]
        return dict(heads=n_heads, pcs=n, max_bb=max_bb, distinct_pcs=n_pcs, distinct_runs=n_runs, superblocks=n_sb, resident_heads=resident,
                    runs={k: stats(v) for k, v in times.items()}, ns_per_head_median=round(statistics.median(times["detect"]) * 1e6 / n_heads, 2),
                    detect_over_copy=ratio("detect", "copy"), detect_over_sort=ratio("detect", "sort"), stages_event_timed=stages,
                    count_two_blocks=dict(occurrences=int(out.value), **stats(count_ms)), levels=run_stats["levels"],
                    jumping_clusters=run_stats["jumping_clusters"], seeds=run_stats["seeds"], run_instances=run_stats["runs"],
                    peak_scratch_bytes=run_stats["peak_bytes"])

    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, blocks=len(blocks), workloads={})
    for lh in args.log_heads:
        for kind in ("hot", "spread", "distinct"):
            for max_bb in args.max_bb:
                key = f"{kind} 2^{lh} max_bb {max_bb}"
                result["workloads"][key] = measure(key, kind, lh, max_bb)
                torch.cuda.empty_cache()
    # hot against spread per head, next to the sort yardstick's own spread (max / min of its runs)
    result["hot_over_spread_per_head"] = {}
    for lh in args.log_heads:
        for max_bb in args.max_bb:
            hot, spread = result["workloads"][f"hot 2^{lh} max_bb {max_bb}"], result["workloads"][f"spread 2^{lh} max_bb {max_bb}"]
            sort = hot["runs"]["sort"]
            result["hot_over_spread_per_head"][f"2^{lh} max_bb {max_bb}"] = dict(
                ratio=round(hot["ns_per_head_median"] / spread["ns_per_head_median"], 2), sort_max_over_min=round(sort["ms_max"] / sort["ms_min"], 2))
    if args.second_route_log_heads:
        lh = args.second_route_log_heads
        pcs = pcs_of(heads_of("hot", lh)).tolist()
        t0 = time.perf_counter()
        want = ref.detect(pcs, blocks, max_bb=4)
        result["second_route_hot"] = dict(heads=1 << lh, max_bb=4, wall_s=round(time.perf_counter() - t0, 2), superblocks=len(want["superblock_counts"]))
    result["not_measured"] = ["the trace route at this size (its index stage is §5p's, measured there)", "count with removal on a hot needle (the doubling tables)",
                              "a scratch bound below the default", "the second route on the spread and distinct workloads (quadratic in Python)",
                              "max_bb above 4"]
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
