"""The memory Merkle AIR's trace generator (pw_memory_merkle_trace, powdr_amd/memory_tree.py merkle_trace). One MI355X, one
process, the runs alternating after a warm-up; the kernel timed by the library's HIP events, whole calls by the host clock around calls
that synchronise themselves. Each section merges its object into --out.
  trace     a tree of 2^--log-stored leaves scattered over the 2^30 key space; updates of 2^12, 2^16 and 2^20 of its leaves:
            merkle_rows_kernel against two yardsticks of the same build and process —
              update   MemoryTree.update with records and node ids for the same keys (the call that makes the kernel's input)
              copy     a device-to-device copy_ of as many bytes as the kernel reads and writes: 105 words per node (its two 25-column
                       record rows and its 55-column row). The kernel does more than those 105 words: it reads two 64-bit ids per
                       node, searches the id array (about log2(nodes) dependent loads) and writes the zero rows up to 2^log_height —
                       up to as many again as the nodes. The ratio to the copy is therefore no pure bandwidth efficiency; the
                       profile says so (copy_yardstick) and gives the padding rows of every size.
            A new capability has no parent figure: both ratios are recorded with min .. max over the steps, nothing is asserted.
  prove     prove_segment of {a stand-in for the boundary AIR's leaf sends, the Merkle AIR, the Poseidon2 chip} for an update of
            2^--prove-log-touched leaves, interpreted (POWDR_JIT=0) and specialised (POWDR_JIT=1), the same words

  python tools/bench_memory_merkle.py --section trace|prove [--steps 3] [--warmup 1] [--out profiles/memory_merkle.json]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
P = 0x78000001
H = 30
WORDS_PER_NODE = 2 * 25 + 55


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", required=True, choices=["trace", "prove"])
    ap.add_argument("--log-stored", type=int, default=20)
    ap.add_argument("--touched", type=int, nargs="*", default=[12, 16, 20])
    ap.add_argument("--prove-log-touched", type=int, default=12)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "memory_merkle.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_memory_merkle: needs a GPU")
    from powdr_amd import abi, prover
    from powdr_amd import memory_tree as mt
    from powdr_amd import system_airs as sa

    note = lambda *a: print("[bench_memory_merkle]", *a, file=sys.stderr, flush=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ts):
        return dict(ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), ms_all=[round(t, 4) for t in ts])

    def ratio(a, b):
        """a / b over the steps: the medians', and the least and the most the steps allow"""
        return dict(median=round(statistics.median(a) / statistics.median(b), 4), min=round(min(a) / max(b), 4), max=round(max(a) / min(b), 4))

    def words(n, seed, leaf=False):
        g = torch.Generator(device="cuda").manual_seed(seed)
        w = torch.randint(0, P, (n, 8), dtype=torch.int32, device="cuda", generator=g)  # (any word below p is a Montgomery word)
        if leaf:  # what a leaf of the memory holds: four words, then zeros
            w[:, 4:] = 0
        return w

    rng = np.random.default_rng(5)
    n = 1 << args.log_stored
    host_keys = np.unique(rng.integers(0, 1 << H, int(1.05 * n) + 64, dtype=np.uint64))
    host_keys = np.sort(rng.choice(host_keys, n, replace=False))
    keys = torch.from_numpy(host_keys.view(np.int64)).cuda()
    pay = words(n, 3, leaf=True)
    tree = mt.MemoryTree(H)
    assert tree.load(keys, pay) == (0, 0)
    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, log_stored=args.log_stored, words_per_node=WORDS_PER_NODE)
    section = {}

    def touched_set(log_touched, seed):
        m = 1 << log_touched
        at = torch.from_numpy(np.sort(np.random.default_rng(seed).choice(n, m, replace=False))).cuda()
        return keys[at].contiguous(), pay[at].contiguous(), words(m, 40 + log_touched, leaf=True)

    if args.section == "trace":
        for log_touched in args.touched:
            tk, a, b = touched_set(log_touched, 7 + log_touched)
            state = [a, b]  # the payloads go a -> b -> a

            def update():
                r = tree.update(tk, state[0], state[1], node_ids=True, cap_log_height=cap, out=rec_out)
                assert r[0] == 0, r[:2]
                state.reverse()
                return r

            cap = 10
            rec_out = None
            r = update()  # (sizes: the wrapper retries at the height the library asks for)
            cap, rows = r[3], r[4]
            rec_out = torch.empty(25 << cap, dtype=torch.int32, device="cuda")
            nodes = rows // 2
            mlh = max(1, (nodes - 1).bit_length())
            out = torch.empty(55 << mlh, dtype=torch.int32, device="cuda")
            src = torch.empty(WORDS_PER_NODE * 4 * nodes // 2, dtype=torch.uint8, device="cuda")  # read + written = 105 words per node
            dst = torch.empty_like(src)
            last = {}

            def trace_call():
                records, ids = last["update"][2]
                got = mt.merkle_trace(records, ids, last["update"][3], last["update"][4], H, cap_log_height=mlh, out=out)
                assert got[1:] == (mlh, nodes, 0), got[1:]
                return got

            def kernel():
                abi.lib.powdr_gpu_timing_enable(1)
                trace_call()
                torch.cuda.synchronize()
                ms = abi.timing_report()["memory_merkle_rows_kernel"]
                abi.lib.powdr_gpu_timing_enable(0)
                assert ms[0] == 1
                return ms[1]

            def copy():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dst.copy_(src)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)

            ts = dict(update=[], trace_call=[], kernel=[], copy=[])
            for it in range(args.warmup + args.steps):
                dt, last["update"] = timed(update)  # (first: the other three read its records)
                order = ["trace_call", "kernel", "copy"]
                got = {"update": dt}
                for name in (order if it % 2 == 0 else order[::-1]):
                    got[name] = timed(trace_call)[0] if name == "trace_call" else kernel() if name == "kernel" else copy()
                note(log_touched, it, {k: round(v, 4) for k, v in got.items()})
                if it >= args.warmup:
                    for k, v in got.items():
                        ts[k].append(v)
            bytes_moved = WORDS_PER_NODE * 4 * nodes
            cell = dict(nodes=nodes, n_rows=rows, records_log_height=cap, log_height=mlh, padding_rows=(1 << mlh) - nodes, search_steps=nodes.bit_length(),
                        bytes_read_and_written=bytes_moved,
                        update_with_records_and_ids=stats(ts["update"]), merkle_trace_call=stats(ts["trace_call"]), merkle_rows_kernel=stats(ts["kernel"]),
                        device_copy=stats(ts["copy"]),
                        kernel_gb_per_second=round(bytes_moved / statistics.median(ts["kernel"]) / 1e6, 1),
                        device_copy_gb_per_second=round(bytes_moved / statistics.median(ts["copy"]) / 1e6, 1),
                        # the first ratio: what the Merkle trace adds to the update that makes its input; the second: the kernel's rate
                        # as a fraction of the copy's (copy ms / kernel ms)
                        trace_call_over_update=ratio(ts["trace_call"], ts["update"]), kernel_over_update=ratio(ts["kernel"], ts["update"]),
                        kernel_rate_over_copy_rate=ratio(ts["copy"], ts["kernel"]))
            section[f"2^{log_touched}"] = cell
            note(log_touched, cell)
            if len(state) and state[0] is not a:  # an even number of updates: the tree holds the image's payloads again
                update()
            del rec_out, out, src, dst, last
            torch.cuda.empty_cache()

    if args.section == "prove":
        from powdr_amd import periphery

        tk, a, b = touched_set(args.prove_log_touched, 99)
        root_before = tree.root()
        status, info, (records, ids), lh, rows = tree.update(tk, a, b, node_ids=True)
        assert status == 0
        trace, mlh, nodes, status = mt.merkle_trace(records, ids, lh, rows, H)
        assert status == 0
        m = tk.numel()
        leaf_lh = max(1, (m - 1).bit_length())
        # [is_valid, key, init0..3, fin0..3] in Montgomery form: the payload words are the Montgomery words the tree was given
        r_mod_p = (1 << 32) % P
        leaf = torch.zeros((10, 1 << leaf_lh), dtype=torch.int32, device="cuda")
        leaf[0, :m] = r_mod_p
        leaf[1, :m] = ((tk * r_mod_p) % P).to(torch.int32)
        leaf[2:6, :m] = a[:, :4].t()
        leaf[6:10, :m] = b[:, :4].t()
        leaf = leaf.reshape(-1).contiguous()
        leaf_inter = periphery._tables(mt.BUS_LEAF, [(periphery._col(0), [periphery._col(1 + j) for j in range(9)])])
        no_cons = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))
        air, chip_air = mt.merkle_air(H), sa.poseidon2_air()
        public = np.concatenate([root_before, tree.root()]).astype(np.uint32)
        runs = {}
        for mode in ("0", "1"):
            os.environ["POWDR_JIT"] = mode
            ps = [prover.Prover(10, *no_cons, num_queries=args.queries, interactions=leaf_inter), air.make_prover(args.queries), chip_air.make_prover(args.queries)]
            ps[1].set_public_values(public)
            senders = [(ps[0], leaf.data_ptr(), leaf_lh), (ps[1], trace.data_ptr(), mlh)]
            chip_trace, chip_lh, chip_rows, status = sa.poseidon2_compress_trace(senders, 10)
            assert status == 0
            seg = senders + [(ps[2], chip_trace.data_ptr(), chip_lh)]
            if mode == "0":
                summaries, _ = prover.check_segment_buses(seg, buses=[5, 8, 9])
                assert all(s["status"] == 0 for s in summaries), summaries
                assert ps[1].check_constraints(trace.data_ptr(), mlh) == (0, None, None)
            ts, proof = [], None
            for it in range(args.warmup + args.steps):
                dt, proof = timed(lambda: prover.prove_segment(seg, logup=True))
                note("prove", mode, it, round(dt, 2), "ms")
                if it >= args.warmup:
                    ts.append(dt)
            runs[mode] = (ts, proof, [p.specialised()["state"] for p in ps])
            for p in ps:
                p.close()
        os.environ.pop("POWDR_JIT", None)
        assert len(runs["0"][1]) == len(runs["1"][1]) and (runs["0"][1] == runs["1"][1]).all()
        section.update(log_touched=args.prove_log_touched, nodes=nodes, merkle_log_height=mlh, leaf_log_height=leaf_lh, chip_rows=chip_rows, chip_log_height=chip_lh,
                       queries=args.queries, proof_words=int(len(runs["0"][1])), interpreted=stats(runs["0"][0]), specialised=stats(runs["1"][0]),
                       specialised_states=runs["1"][2], interpreted_over_specialised=ratio(runs["0"][0], runs["1"][0]))

    tree.close()
    out = Path(args.out)
    if out.exists():
        result = {**json.loads(out.read_text()), **result}
    result[args.section] = section
    result["copy_yardstick"] = ("105 words per node: the two 25-column record rows read and the 55-column row written. Not counted, and done by the kernel: two "
                                "64-bit ids read per node, a binary search of search_steps dependent loads in the id array, and 55 zero words for each "
                                "of padding_rows. kernel_rate_over_copy_rate is therefore not a pure bandwidth efficiency")
    result["not_measured"] = ["rows written straight from pw_memory_tree_update without the 25-column records in between",
                              "trees of other heights than 30, dense keys", "other streams, more than one update in flight, multi-GPU",
                              "the chained VM's segments (a few thousand nodes: launch-bound)"]
    print(json.dumps({args.section: section}))
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
