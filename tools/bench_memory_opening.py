"""The memory tree's multi-opening (pw_memory_tree_open, powdr_amd/memory_tree.py MemoryTree.open). One MI355X, one
process, the runs alternating after a warm-up; whole calls by the host clock around calls that synchronise themselves, the opening's
three launches by the library's HIP events. A tree of 2^--log-stored leaves scattered over the 2^30 key space, held twice (one tree per
mode); openings of 2^4, 2^12, 2^16 and 2^20 of its leaves against two yardsticks of the same build and process —
  update   MemoryTree.update(keys, init == fin, records=True, node_ids=True) of the same keys, on the rebuild-mode tree and on the
           incremental one: the only way to get these digests before the opening existed (they are among the 25-column records)
  copy     a device-to-device copy_ of as many bytes as the opening writes — 32 per key and 32 per sibling — which is also what it
           reads of payloads and digests. Not counted, and done by the opening: the keys read once per level, a flag byte and a 64-bit
           rank per (level, key) written, scanned and read again, and about log2(level size) dependent loads per emitted sibling.
           The ratio to the copy is therefore no pure bandwidth efficiency.
A new capability has no parent figure: the ratios are recorded as median (min .. max) over the steps, nothing is asserted.

  python tools/bench_memory_opening.py [--steps 3] [--warmup 1] [--out profiles/memory_opening.json]"""
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
KERNELS = ("memory_tree_open_flag_kernel", "memory_tree_open_scan", "memory_tree_open_gather_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-stored", type=int, default=20)
    ap.add_argument("--opened", type=int, nargs="*", default=[4, 12, 16, 20])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "memory_opening.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_memory_opening: needs a GPU")
    from powdr_amd import abi
    from powdr_amd import memory_tree as mt

    note = lambda *a: print("[bench_memory_opening]", *a, file=sys.stderr, flush=True)

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

    rng = np.random.default_rng(5)
    n = 1 << args.log_stored
    host_keys = np.unique(rng.integers(0, 1 << H, int(1.05 * n) + 64, dtype=np.uint64))
    host_keys = np.sort(rng.choice(host_keys, n, replace=False))
    keys = torch.from_numpy(host_keys.view(np.int64)).cuda()
    g = torch.Generator(device="cuda").manual_seed(3)
    pay = torch.randint(0, P, (n, 8), dtype=torch.int32, device="cuda", generator=g)  # (any word below p is a Montgomery word)
    trees = {"rebuild": mt.MemoryTree(H), "incremental": mt.MemoryTree(H, incremental=True)}
    for t in trees.values():
        assert t.load(keys, pay) == (0, 0)
    root = trees["rebuild"].root()
    assert (trees["incremental"].root() == root).all()
    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, log_stored=args.log_stored, height=H,
                  stored_nodes=trees["rebuild"].stats()["stored_nodes"])
    section = {}
    for log_opened in args.opened:
        m_keys = 1 << log_opened
        at = torch.from_numpy(np.sort(np.random.default_rng(7 + log_opened).choice(n, m_keys, replace=False))).cuda()
        ok, op = keys[at].contiguous(), pay[at].contiguous()
        status, info, d_pay, d_sib = trees["rebuild"].open(ok, device=True)  # (sizes: the wrapper retries with the count the library asks for)
        assert (status, info) == (0, 0) and torch.equal(d_pay, op)
        n_sib = d_sib.shape[0]
        if log_opened <= 16:  # the opening is an opening of this tree's root
            to_host = lambda t: mt._from_monty(t.cpu().numpy().view(np.uint32))
            code = mt.verify_opening(H, root, ok.cpu().numpy().view(np.uint64), to_host(d_pay), to_host(d_sib))
            assert code == (0, 0), code
        del d_pay, d_sib
        caps, outs = {}, {}
        for mode, t in trees.items():
            r = t.update(ok, op, op, node_ids=True)
            assert r[0] == 0 and (t.root() == root).all(), r[:2]
            caps[mode] = r[3]
            del r
        rows = None
        rec_out = torch.empty(25 << max(caps.values()), dtype=torch.int32, device="cuda")
        moved = 32 * (m_keys + n_sib)
        src = torch.empty(moved, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def opening():
            r = trees["rebuild"].open(ok, cap_siblings=n_sib, device=True)
            assert r[0] == 0 and r[3].shape[0] == n_sib
            return r

        def kernels():
            abi.lib.powdr_gpu_timing_enable(1)
            opening()
            torch.cuda.synchronize()
            ms = abi.timing_report()
            abi.lib.powdr_gpu_timing_enable(0)
            assert all(ms[k][0] == 1 for k in KERNELS), ms
            return {k: ms[k][1] for k in KERNELS}

        def update(mode):
            r = trees[mode].update(ok, op, op, node_ids=True, cap_log_height=caps[mode], out=rec_out)
            assert r[0] == 0
            return r[4]

        def copy():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        ts = {k: [] for k in ("open_call", "open_kernels", "update_rebuild", "update_incremental", "copy") + KERNELS}
        order = ["open_call", "open_kernels", "update_rebuild", "update_incremental", "copy"]
        for it in range(args.warmup + args.steps):
            got = {}
            for name in (order if it % 2 == 0 else order[::-1]):
                if name == "open_call":
                    got[name] = timed(opening)[0]
                elif name == "open_kernels":
                    ks = kernels()
                    got.update(ks)
                    got[name] = sum(ks.values())
                elif name == "copy":
                    got[name] = copy()
                else:
                    got[name], rows = timed(lambda: update(name.split("_")[1]))
            note(log_opened, it, {k: round(v, 4) for k, v in got.items()})
            if it >= args.warmup:
                for k, v in got.items():
                    ts[k].append(v)
        for t in trees.values():
            assert (t.root() == root).all()
        cell = dict(keys=m_keys, siblings=n_sib, siblings_per_key=round(n_sib / m_keys, 2), lanes=m_keys * H, update_record_rows=rows,
                    bytes_written=moved, scratch_bytes=9 * (m_keys * H + 1),
                    open_call=stats(ts["open_call"]), open_launches=stats(ts["open_kernels"]), **{k: stats(ts[k]) for k in KERNELS},
                    update_with_records_and_ids_rebuild=stats(ts["update_rebuild"]), update_with_records_and_ids_incremental=stats(ts["update_incremental"]),
                    device_copy=stats(ts["copy"]),
                    open_launches_gb_per_second=round(moved / statistics.median(ts["open_kernels"]) / 1e6, 1),
                    device_copy_gb_per_second=round(moved / statistics.median(ts["copy"]) / 1e6, 1),
                    # how many times the opening fits into the update that gave these digests before; the launches' rate as a fraction of the copy's
                    update_rebuild_over_open_call=ratio(ts["update_rebuild"], ts["open_call"]),
                    update_incremental_over_open_call=ratio(ts["update_incremental"], ts["open_call"]),
                    open_rate_over_copy_rate=ratio(ts["copy"], ts["open_kernels"]), call_rate_over_copy_rate=ratio(ts["copy"], ts["open_call"]))
        section[f"2^{log_opened}"] = cell
        note(log_opened, cell)
        del rec_out, src, dst
        torch.cuda.empty_cache()
    for t in trees.values():
        t.close()
    result["openings"] = section
    result["copy_yardstick"] = ("32 bytes per key and per sibling, read and written: what the opening writes, and what it reads of payloads and digests. Not counted, "
                                "and done by the opening: the keys once per level, a flag byte and a 64-bit rank per (level, key) written, scanned and read "
                                "again (scratch_bytes), and a binary search of dependent loads per sibling. open_rate_over_copy_rate is therefore no pure "
                                "bandwidth efficiency")
    result["not_measured"] = ["trees of other heights than 30, dense keys, keys that are not stored", "other streams, more than one opening in flight, multi-GPU",
                              "the host verifier (pw_memory_opening_verify: one permutation per key and per node of the touched sets)",
                              "the chained VM's openings (a few keys: launch-bound, the 2^4 row)"]
    print(json.dumps({"openings": section}))
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
