"""The sparse memory Merkle tree (pw_memory_tree_*, powdr_amd/memory_tree.py). One process per section, the measurements
alternating after a warm-up, host clock around calls that synchronise themselves; per-kernel times from the library's HIP events. Each
section merges its object into --out, so that a job can run every section under a time limit of its own. `sizes` and `segment` measure
every mode of --modes (rebuild: every level hashed again; incremental: only the touched paths, pw_memory_tree_set_mode) on trees of their
own, alternating; --parent names the file the PARENT commit's copy of this tool wrote in the same job (its only mode is the rebuild):
its figures are put next to each cell, with parent's fastest step over this build's slowest.
  kernel    (a) permutations per second of memory_tree_level_kernel while 2^log_leaves dense leaves are loaded, against compress_kernel
            committing a matrix of as many rows (pw_merkle_commit), alternating
  sizes     trees of 2^20 and 2^24 stored leaves, dense keys and keys scattered over the whole 2^30 space (the worst case for stored
            nodes: bytes held), updates of 2^12, 2^16 and 2^20 stored leaves with and without records: ms, permutations hashed against
            the permutations on the touched paths, launches, host read-backs, peak scratch, per-kernel ms of one more update with
            the library's events on; at the smallest update also move_kernel's bytes per second (read + written) against a
            device-to-device copy of as many bytes
  segment   (b) the memory-log segment of tools/bench_system_airs.py: boundary trace -> boundary_leaves -> update, as a fraction of
            that segment's prove_segment

  python tools/bench_memory_tree.py --section kernel|sizes|segment [--steps 3] [--warmup 1] [--modes rebuild incremental]
         [--parent parent.json] [--out profiles/memory_tree_incremental.json]
profiles/memory_tree.json is the record of the commit that added the tree (rebuild only) and is not written any more."""
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
    ap.add_argument("--modes", nargs="*", default=["rebuild", "incremental"], choices=["rebuild", "incremental"])
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "memory_tree_incremental.json"))
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

    def stored_level_sizes(keys):
        """s_l of the tree over these sorted device keys, l = 0 .. H"""
        out, t = [keys.numel()], keys
        for _ in range(H):
            t = torch.unique_consecutive(t >> 1)
            out.append(t.numel())
        return out

    def over_parent(cell, parent_cell):
        """the parent's figures next to this build's, and parent's fastest step over this build's slowest (and the medians')"""
        for k in ("with_records", "without_records"):
            cell["parent"][k] = parent_cell[k]
            for mode in args.modes:
                cell[mode][k + "_parent_min_over_max"] = round(parent_cell[k]["ms_min"] / cell[mode][k]["ms_max"], 3)
                cell[mode][k + "_parent_median_over_median"] = round(parent_cell[k]["ms_median"] / cell[mode][k]["ms_median"], 3)

    parent = json.loads(Path(args.parent).read_text()) if args.parent else None
    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, tail_nodes=mt.TAIL_NODES, modes=args.modes)
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
                trees, ms_load = {}, {}
                for mode in args.modes:
                    trees[mode] = mt.MemoryTree(H, incremental=mode == "incremental")
                    ms_load[mode], st = timed(lambda: trees[mode].load(keys, pay))
                    assert st == (0, 0)
                s0 = trees[args.modes[0]].stats()
                stored = stored_level_sizes(keys)
                merged = sum(1 for l in range(1, H + 1) if stored[l - 1] > mt.TAIL_NODES)  # L: the levels with launches of their own
                assert s0["stored_nodes"] == sum(stored)
                entry = dict(load_ms={m: round(v, 3) for m, v in ms_load.items()}, leaves=s0["leaves"], stored_nodes=s0["stored_nodes"], device_bytes=s0["device_bytes"],
                             bytes_per_leaf=round(s0["device_bytes"] / n, 1), load_permutations=s0["last_permutations"], load_launches=s0["last_launches"],
                             levels_above_the_tail_threshold=merged, updates={})
                note(log_stored, layout, entry)
                for log_touched in args.touched:
                    m = 1 << log_touched
                    if m > n:
                        continue
                    at = np.sort(rng.choice(n, m, replace=False))
                    tk = keys[torch.from_numpy(at).cuda()].contiguous()
                    words_a, words_b = pay[torch.from_numpy(at).cuda()].contiguous(), words(m, 4 + log_touched)
                    touched = level_sizes(host_keys[at])
                    touched_perms = sum(touched)
                    touched_above = sum(1 for l in range(1, H + 1) if touched[l - 1] > mt.TAIL_NODES)
                    cap = max(1, (2 * touched_perms - 1).bit_length())
                    out = torch.empty(25 << cap, dtype=torch.int32, device="cuda")
                    state = {mode: [words_a, words_b] for mode in args.modes}  # the payloads go a -> b -> a, per tree

                    def update(mode, rec):
                        a, b = state[mode]
                        r = trees[mode].update(tk, a, b, records=rec, cap_log_height=cap, out=out if rec else None)
                        assert r[0] == 0, r[:2]
                        state[mode] = [b, a]
                        return r

                    ts = {mode: dict(with_records=[], without_records=[]) for mode in args.modes}
                    last = None
                    for it in range(2 * (args.warmup + args.steps)):  # with records, without, alternating; inside, the modes alternating
                        rec = it % 2 == 0
                        for mode in (args.modes if (it // 2) % 2 == 0 else args.modes[::-1]):
                            dt, r = timed(lambda: update(mode, rec))
                            if it >= 2 * args.warmup:
                                ts[mode]["with_records" if rec else "without_records"].append(dt)
                            if rec:
                                last = r
                    cell = dict(n_rows=last[4], log_height=last[3], permutations_on_touched_paths=touched_perms, parent={})
                    for mode in args.modes:
                        su = trees[mode].stats()
                        want = m + sum(stored[1:]) if mode == "rebuild" else m + sum(touched[1:merged + 1]) + sum(stored[merged + 1:])
                        assert su["last_permutations"] == want, (mode, su["last_permutations"], want)
                        kern = event_timed(lambda: update(mode, False), ("memory_tree_",))
                        update(mode, False)  # an even number of updates: the tree holds the image's payloads again
                        assert state[mode][0] is words_a
                        cell[mode] = dict(
                            with_records=stats(ts[mode]["with_records"]), without_records=stats(ts[mode]["without_records"]), permutations_hashed=su["last_permutations"],
                            hashed_over_touched=round(su["last_permutations"] / touched_perms, 2), launches=su["last_launches"],
                            # validate, continuity, a count per touched set above the threshold and the tail's sets, a count per level above it and the tail
                            host_read_backs=4 + touched_above + merged, peak_scratch_bytes=su["last_scratch_bytes"], kernels_without_records=kern)
                    if "incremental" in args.modes and log_touched == min(args.touched):
                        moved = sum(stored[l] - touched[l] for l in range(1, merged + 1))  # every key is stored: T_l is part of the old level
                        ms_move = cell["incremental"]["kernels_without_records"]["memory_tree_move_kernel"]["ms"]
                        src = torch.empty(moved * 40, dtype=torch.uint8, device="cuda")
                        dst = torch.empty_like(src)
                        copies = []
                        for _ in range(args.warmup + args.steps):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            dst.copy_(src)
                            e1.record()
                            torch.cuda.synchronize()
                            copies.append(e0.elapsed_time(e1))
                        ms_copy = statistics.median(copies[args.warmup:])
                        cell["move_kernel"] = dict(nodes_moved=moved, bytes_read_and_written=2 * 40 * moved, launches=merged, ms=ms_move,
                                                   gb_per_second=round(2 * 40 * moved / ms_move / 1e6, 1), device_copy_ms=round(ms_copy, 4),
                                                   device_copy_ms_all=[round(x, 4) for x in copies[args.warmup:]],
                                                   device_copy_gb_per_second=round(2 * 40 * moved / ms_copy / 1e6, 1), over_device_copy=round(ms_copy / ms_move, 3))
                        del src, dst
                    if parent:
                        over_parent(cell, parent["sizes"][f"2^{log_stored}_{layout}"]["updates"][f"2^{log_touched}"])
                    entry["updates"][f"2^{log_touched}"] = cell
                    note(log_stored, layout, log_touched, cell)
                    del out
                section[f"2^{log_stored}_{layout}"] = entry
                for t in trees.values():
                    t.close()
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
        trees = {mode: mt.MemoryTree(H, incremental=mode == "incremental") for mode in args.modes}
        for t in trees.values():
            assert t.load(keys, init) == (0, 0)
        rec_cap = 27
        out = torch.empty(25 << rec_cap, dtype=torch.int32, device="cuda")
        state = {mode: [init, fin] for mode in args.modes}

        def update(mode, records):
            a, b = state[mode]
            r = trees[mode].update(keys, a, b, records=records, cap_log_height=rec_cap, out=out if records else None)
            assert r[0] == 0, r[:2]
            state[mode] = [b, a]
            return r

        runs = {"boundary_leaves": lambda: mt.boundary_leaves(trace, lh, locations)}
        for mode in args.modes:
            runs[f"update_with_records_{mode}"] = lambda mode=mode: update(mode, True)
            runs[f"update_without_records_{mode}"] = lambda mode=mode: update(mode, False)
        runs.update({"memory_boundary_trace": lambda: sa.memory_boundary_trace(seg, cap), "prove_segment": lambda: prover.prove_segment(seg, logup=True, copy=False)})
        times, last = {k: [] for k in runs}, {}
        for it in range(args.warmup + args.steps):
            for k in (list(runs) if it % 2 == 0 else list(runs)[::-1]):
                dt, last[k] = timed(runs[k])
                if it >= args.warmup:
                    times[k].append(dt)
                note(it, k, round(dt, 2), "ms")
        first = args.modes[0]
        section.update(log_rows=args.log_rows, locations=locations, runs={k: stats(v) for k, v in times.items()}, n_rows=last[f"update_with_records_{first}"][4],
                       record_log_height=last[f"update_with_records_{first}"][3], tree={mode: t.stats() for mode, t in trees.items()})
        section["kernels_without_records"] = {mode: event_timed(lambda: update(mode, False), ("memory_tree_",)) for mode in args.modes}
        prove = section["runs"]["prove_segment"]["ms_median"]
        section["fraction_of_prove_segment"] = {k: round(v["ms_median"] / prove, 4) for k, v in section["runs"].items() if k != "prove_segment"}
        if parent:
            section["parent"] = {k: parent["segment"]["runs"][k] for k in ("update_with_records", "update_without_records", "prove_segment")}
            for mode in args.modes:
                for k in ("update_with_records", "update_without_records"):
                    mine, theirs = section["runs"][f"{k}_{mode}"], section["parent"][k]
                    section[f"{k}_{mode}_parent_min_over_max"] = round(theirs["ms_min"] / mine["ms_max"], 3)
                    section[f"{k}_{mode}_parent_median_over_median"] = round(theirs["ms_median"] / mine["ms_median"], 3)
        for t in trees.values():
            t.close()
        for p in provers:
            p.close()

    out = Path(args.out)
    if out.exists():
        result = {**json.loads(out.read_text()), **result}
    result[args.section] = section
    result["not_measured"] = ["an in-place incremental update (the new levels are built next to the old ones, as in the rebuild)",
                              "trees of other heights than 30", "more than one update in flight, other streams, multi-GPU",
                              "the tree under a device budget (pw_set_device_budget does not account for it)",
                              "the chained VM's segments (a few thousand locations: launch-bound, see the launches per update)"]
    print(json.dumps({args.section: section}))
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
