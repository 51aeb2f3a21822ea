"""The sparse memory Merkle tree (pw_memory_tree_*, powdr_amd/memory_tree.py). A new capability has no parent figure, so
it is reported against two yardsticks of the same build. One process per section, the measurements alternating after a warm-up, host
clock around calls that synchronise themselves; per-kernel times from the library's HIP events. Each section merges its object into
--out, so that a job can run every section under a time limit of its own:
  kernel    (a) permutations per second of memory_tree_level_kernel while 2^log_leaves dense leaves are loaded, against compress_kernel
            committing a matrix of as many rows (pw_merkle_commit), alternating
  sizes     trees of 2^20 and 2^24 stored leaves, dense keys and keys scattered over the whole 2^30 space (the worst case for stored
            nodes: bytes held), updates of 2^12, 2^16 and 2^20 stored leaves with and without records: ms, permutations hashed against
            the permutations on the touched paths (what an incremental rebuild would hash), launches, peak scratch
  segment   (b) the memory-log segment of tools/bench_system_airs.py: boundary trace -> boundary_leaves -> update, as a fraction of
            that segment's prove_segment

  python tools/bench_memory_tree.py --section kernel|sizes|segment [--steps 3] [--warmup 1] [--out profiles/memory_tree.json]"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
P = 0x78000001
H = 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", required=True, choices=["kernel", "sizes", "segment"])
    ap.add_argument("--log-leaves", type=int, default=20)
    ap.add_argument("--stored", type=int, nargs="*", default=[20, 24])
    ap.add_argument("--touched", type=int, nargs="*", default=[12, 16, 20])
    ap.add_argument("--log-rows", type=int, default=24)
    ap.add_argument("--locations", type=int, default=4000000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "memory_tree.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_memory_tree: needs a GPU")
    from powdr_amd import abi, prover
    from powdr_amd import memory_tree as mt

    note = lambda *a: print("[bench_memory_tree]", *a, file=sys.stderr, flush=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ts):
        return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), ms_all=[round(t, 3) for t in ts])

    def event_timed(fn, prefixes):
        abi.lib.powdr_gpu_timing_enable(1)
        fn()
        torch.cuda.synchronize()
        kern = {k: dict(launches=v[0], ms=round(v[1], 4)) for k, v in abi.timing_report().items() if k.startswith(prefixes)}
        abi.lib.powdr_gpu_timing_enable(0)
        return kern

    def words(n, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        return torch.randint(0, P, (n, 8), dtype=torch.int32, device="cuda", generator=g)  # (any word below p is a Montgomery word)

    def level_sizes(keys):
        """|T_l| of a sorted key set, l = 0 .. H"""
        out, t = [len(keys)], keys
        for _ in range(H):
            t = np.unique(t >> np.uint64(1))
            out.append(len(t))
        return out

    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, tail_nodes=mt.TAIL_NODES)
    section = {}

    if args.section == "kernel":
        n = 1 << args.log_leaves
        keys = torch.arange(n, dtype=torch.int64, device="cuda")
        pay = words(n, 1)
        leaves = words(n, 2).t().contiguous().reshape(-1)  # an 8-column matrix of n rows for pw_merkle_commit
        digs = torch.empty((2 * n - 1) * 8, dtype=torch.int32, device="cuda")
        tail = mt.TAIL_NODES

        def load():
            t = mt.MemoryTree(H)
            assert t.load(keys, pay) == (0, 0)
            t.close()

        commit = lambda: abi.check(prover.lib.pw_merkle_commit(leaves.data_ptr(), n, 8, digs.data_ptr()), "pw_merkle_commit")
        level_perms = sum(n >> l for l in range(1, args.log_leaves + 1) if n >> (l - 1) > tail)  # parents of levels above the tail
        compress_perms = sum(n >> l for l in range(1, args.log_leaves + 1) if n >> (l - 1) > 2048)  # merkle.hip kTailNodes
        rates = dict(level=[], compress=[], leaf=[])
        for it in range(args.warmup + args.steps):
            order = [("tree", load), ("commit", commit)]
            for name, fn in (order if it % 2 == 0 else order[::-1]):
                kern = event_timed(fn, ("memory_tree_", "compress_kernel"))
                note(it, name, kern)
                if it < args.warmup:
                    continue
                if name == "tree":
                    rates["level"].append(level_perms / (kern["memory_tree_level_kernel"]["ms"] * 1e-3))
                    rates["leaf"].append(n / (kern["memory_tree_leaf_kernel"]["ms"] * 1e-3))
                    section["tree_kernels"] = kern
                else:
                    rates["compress"].append(compress_perms / (kern["compress_kernel"]["ms"] * 1e-3))
                    section["commit_kernels"] = kern
        med = {k: statistics.median(v) for k, v in rates.items()}
        section.update(log_leaves=args.log_leaves, level_kernel_permutations=level_perms, compress_kernel_permutations=compress_perms,
                       permutations_per_second={k: round(v) for k, v in med.items()}, permutations_per_second_all={k: [round(x) for x in v] for k, v in rates.items()},
                       level_kernel_over_compress_kernel=round(med["level"] / med["compress"], 4))

    if args.section == "sizes":
        rng = np.random.default_rng(5)
        for log_stored in args.stored:
            n = 1 << log_stored
            for layout in ("dense", "scattered"):
                if layout == "dense":
                    host_keys = np.uint64(0x2000000) + np.arange(n, dtype=np.uint64)
                else:
                    host_keys = np.unique(rng.integers(0, 1 << H, int(1.05 * n) + 64, dtype=np.uint64))
                    host_keys = np.sort(rng.choice(host_keys, n, replace=False))
                keys = torch.from_numpy(host_keys.view(np.int64)).cuda()
                pay = words(n, 3)
                tree = mt.MemoryTree(H)
                ms_load, st = timed(lambda: tree.load(keys, pay))
                assert st == (0, 0)
                s0 = tree.stats()
                entry = dict(load_ms=round(ms_load, 3), leaves=s0["leaves"], stored_nodes=s0["stored_nodes"], device_bytes=s0["device_bytes"],
                             bytes_per_leaf=round(s0["device_bytes"] / n, 1), load_permutations=s0["last_permutations"], load_launches=s0["last_launches"],
                             load_permutations_per_second=round(s0["last_permutations"] / (ms_load * 1e-3)), updates={})
                note(log_stored, layout, entry)
                for log_touched in args.touched:
                    m = 1 << log_touched
                    if m > n:
                        continue
                    at = np.sort(rng.choice(n, m, replace=False))
                    tk = keys[torch.from_numpy(at).cuda()].contiguous()
                    a, b = pay[torch.from_numpy(at).cuda()].contiguous(), words(m, 4 + log_touched)
                    touched_perms = sum(level_sizes(host_keys[at]))
                    cap = max(1, (2 * touched_perms - 1).bit_length())
                    out = torch.empty(25 << cap, dtype=torch.int32, device="cuda")
                    ts, plain, last = [], [], None
                    for it in range(2 * (args.warmup + args.steps)):  # with records, without, alternating; the payloads go a -> b -> a
                        rec = it % 2 == 0
                        dt, r = timed(lambda: tree.update(tk, a, b, records=rec, cap_log_height=cap, out=out if rec else None))
                        assert r[0] == 0, r[:2]
                        a, b = b, a
                        if it >= 2 * args.warmup:
                            (ts if rec else plain).append(dt)
                        if rec:
                            last = r
                    su = tree.stats()
                    entry["updates"][f"2^{log_touched}"] = dict(
                        with_records=stats(ts), without_records=stats(plain), n_rows=last[4], log_height=last[3], permutations_hashed=su["last_permutations"],
                        permutations_on_touched_paths=touched_perms, hashed_over_touched=round(su["last_permutations"] / touched_perms, 2), launches=su["last_launches"],
                        peak_scratch_bytes=su["last_scratch_bytes"], permutations_per_second=round(su["last_permutations"] / (statistics.median(plain) * 1e-3)))
                    note(log_stored, layout, log_touched, entry["updates"][f"2^{log_touched}"])
                    del out
                section[f"2^{log_stored}_{layout}"] = entry
                tree.close()
                del keys, pay
                torch.cuda.empty_cache()

    if args.section == "segment":
        from oracle import apc_model as om
        from powdr_amd import periphery
        from powdr_amd import system_airs as sa
        from tests import _system_airs_ref as ref

        no_cons = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))
        to_dev = lambda a: torch.from_numpy(om.to_monty(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)).view(np.int32)).cuda()
        t0 = time.perf_counter()
        cols, want = ref.memory_log(args.log_rows, args.locations, seed=1)
        rng = np.random.default_rng(9)
        rows_t = 1 << 13
        table = rng.integers(0, om.P, size=(9, rows_t)).astype(np.uint32)
        table[0] = 0x1000 + 4 * np.arange(rows_t)
        pick = rng.integers(0, rows_t, size=1 << args.log_rows)
        pick[: 1 << (args.log_rows - 1)] %= 24
        fetch = np.concatenate([table[:, pick], np.ones((1, 1 << args.log_rows), np.uint32)])
        col = periphery._col
        fetch_it = periphery._tables(2, [(col(9), [col(j) for j in range(9)])])
        note("memory log built on the host in", round(time.perf_counter() - t0, 1), "s")
        traces = [to_dev(cols), to_dev(fetch)]
        provers = [prover.Prover(13, *no_cons, num_queries=args.queries, interactions=ref.memory_log_interactions()),
                   prover.Prover(10, *no_cons, num_queries=args.queries, interactions=fetch_it)]
        seg = [(p, t.data_ptr(), args.log_rows) for p, t in zip(provers, traces)]
        torch.cuda.synchronize()
        cap = (want.shape[1] - 1).bit_length()
        trace, lh, locations, status = sa.memory_boundary_trace(seg, cap)
        assert status == 0
        keys, init, fin = mt.boundary_leaves(trace, lh, locations)
        tree = mt.MemoryTree(H)
        assert tree.load(keys, init) == (0, 0)
        rec_cap = 27
        out = torch.empty(25 << rec_cap, dtype=torch.int32, device="cuda")
        state = dict(a=init, b=fin)

        def update(records):
            r = tree.update(keys, state["a"], state["b"], records=records, cap_log_height=rec_cap, out=out if records else None)
            assert r[0] == 0, r[:2]
            state["a"], state["b"] = state["b"], state["a"]
            return r

        runs = {"boundary_leaves": lambda: mt.boundary_leaves(trace, lh, locations), "update_with_records": lambda: update(True),
                "update_without_records": lambda: update(False), "memory_boundary_trace": lambda: sa.memory_boundary_trace(seg, cap),
                "prove_segment": lambda: prover.prove_segment(seg, logup=True, copy=False)}
        times, last = {k: [] for k in runs}, {}
        for it in range(args.warmup + args.steps):
            for k in (list(runs) if it % 2 == 0 else list(runs)[::-1]):
                dt, last[k] = timed(runs[k])
                if it >= args.warmup:
                    times[k].append(dt)
                note(it, k, round(dt, 2), "ms")
        su = tree.stats()
        section.update(log_rows=args.log_rows, locations=locations, runs={k: stats(v) for k, v in times.items()}, n_rows=last["update_with_records"][4],
                       record_log_height=last["update_with_records"][3], tree=su)
        prove = section["runs"]["prove_segment"]["ms_median"]
        section["fraction_of_prove_segment"] = {k: round(section["runs"][k]["ms_median"] / prove, 4)
                                                for k in ("boundary_leaves", "update_with_records", "update_without_records", "memory_boundary_trace")}
        tree.close()
        for p in provers:
            p.close()

    out = Path(args.out)
    if out.exists():
        result = {**json.loads(out.read_text()), **result}
    result[args.section] = section
    result["not_measured"] = ["an incremental rebuild (none was built: hashed_over_touched says what it would save in permutations, not in time)",
                              "trees of other heights than 30", "more than one update in flight, other streams, multi-GPU",
                              "the tree under a device budget (pw_set_device_budget does not account for it)",
                              "the chained VM's segments (a few thousand locations: launch-bound, see the launches per update)"]
    print(json.dumps({args.section: section}))
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
