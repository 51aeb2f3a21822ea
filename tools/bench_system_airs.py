"""Device-side trace generation of the system AIRs (pw_program_frequencies, pw_memory_boundary_trace) against what the
same segment costs anyway: its proof, and (chained segment) the instruction AIRs' trace generation from records. A new capability
has no parent figure, so the two generators are reported as FRACTIONS of those. One process, the measurements alternating after a
warm-up, host clock around calls that synchronise themselves; per-kernel times from the library's HIP events. Prints one JSON object
and writes it to --out:
  memory_log   a "memory log" AIR of 2^log_rows accesses (tests/_system_airs_ref.memory_log) + a "fetch log" AIR of as many rows that
               looks up a program of 2^log_table rows, half of its rows in a loop body of 24 instructions at the table's start; and
               the same fetches with the loop body at row 5000, past the kernel's LDS partition (global atomics merged per wave only)
  chained      a chained execution of `--calls` calls (tests/_chained_vm.py): ten instructions of six chips
per segment: ms of both generators, their kernels, address-table slots / occupancy / tables walked, peak scratch, atomics-per-second
of the frequency kernel (LDS and global atomics the kernel counted itself, next to the additions they carry); ms of prove_segment over
the senders; chained: ms of powdr_original_airs_expand. The issue's size is 2^20 calls x about 60 accesses = 2^26 accesses; the log is
built on the host by sorting, which is what limits --log-rows here.

  python tools/bench_system_airs.py [--log-rows 24] [--locations 4000000] [--calls 4096] [--steps 3] [--warmup 1] [--out profiles/system_airs.json]"""
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
    ap.add_argument("--log-rows", type=int, default=24)
    ap.add_argument("--locations", type=int, default=4000000)
    ap.add_argument("--log-table", type=int, default=13)
    ap.add_argument("--calls", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "system_airs.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_system_airs: needs a GPU")
    from oracle import apc_model as om
    from oracle import original_chips as ooc
    from powdr_amd import abi, periphery, prover
    from powdr_amd import original_chips as pc
    from powdr_amd import system_airs as sa
    from tests import _chained_vm as vm
    from tests import _system_airs_ref as ref

    note = lambda *a: print("[bench_system_airs]", *a, file=sys.stderr, flush=True)
    no_cons = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))
    to_dev = lambda a: torch.from_numpy(om.to_monty(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)).view(np.int32)).cuda()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ts):
        return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), ms_all=[round(t, 3) for t in ts])

    def freq_rates(fk, st):
        """what program_freq_kernel did in one event-timed call: the additions (active triples) it was asked for and the atomics it
        issued for them after merging, per second of kernel time; 2.9 G/s is what one atomic per addition reached on 256 hot bins"""
        out = dict(additions=st["additions"], lds_atomics=st["lds_atomics"], global_atomics=st["global_atomics"], rows_x_interactions_walked=st["walked"])
        if fk and fk["ms"] > 0:
            sec = fk["ms"] * 1e-3
            out.update(kernel_ms=fk["ms"], additions_per_second=round(st["additions"] / sec), lds_atomics_per_second=round(st["lds_atomics"] / sec),
                       global_atomics_per_second=round(st["global_atomics"] / sec), additions_per_atomic=round(st["additions"] / max(1, st["lds_atomics"] + st["global_atomics"]), 2),
                       hot_bin_global_atomics_per_second_r01_microbench=2.9e9)
        return out

    def measure(name, seg, d_table, log_table, pc_base, pc_step, cap, extra):
        """seg: [(Prover, pointer, log_height)] of the senders"""
        runs = {
            "program_frequencies": lambda: sa.program_frequencies(seg, d_table, log_table, pc_base, pc_step),
            "memory_boundary_trace": lambda: sa.memory_boundary_trace(seg, cap),
            "prove_segment": lambda: prover.prove_segment(seg, logup=True, copy=False),
        }
        runs.update(extra)
        times, last, table, freq_stats = {k: [] for k in runs}, {}, {}, {}
        for it in range(args.warmup + args.steps):
            for k in (list(runs) if it % 2 == 0 else list(runs)[::-1]):
                dt, last[k] = timed(runs[k])
                if k == "memory_boundary_trace":
                    table = sa.last_stats()
                if k == "program_frequencies":
                    freq_stats = sa.last_stats()
                if it >= args.warmup:
                    times[k].append(dt)
                note(name, it, k, round(dt, 2), "ms")
        assert last["program_frequencies"][1] == 0 and last["memory_boundary_trace"][3] == 0
        abi.lib.powdr_gpu_timing_enable(1)
        runs["program_frequencies"]()
        runs["memory_boundary_trace"]()
        torch.cuda.synchronize()
        kern = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in abi.timing_report().items() if k.startswith(("program_", "boundary_"))}
        abi.lib.powdr_gpu_timing_enable(0)
        out = dict(runs={k: stats(v) for k, v in times.items()}, kernels_event_timed=kern, address_table=table,
                   occupancy=round(table["occupied_slots"] / max(1, table["table_slots"]), 4), locations=last["memory_boundary_trace"][2],
                   boundary_log_height=last["memory_boundary_trace"][1], peak_scratch_bytes=dict(memory_boundary_trace=table["peak_bytes"], program_frequencies=freq_stats["peak_bytes"]))
        prove = out["runs"]["prove_segment"]["ms_median"]
        out["fraction_of_prove_segment"] = {k: round(out["runs"][k]["ms_median"] / prove, 4) for k in ("program_frequencies", "memory_boundary_trace")}
        for k in extra:
            out[f"fraction_of_{k}"] = {g: round(out["runs"][g]["ms_median"] / out["runs"][k]["ms_median"], 4)
                                       for g in ("program_frequencies", "memory_boundary_trace")}
        out["program_freq_kernel"] = freq_rates(kern.get("program_freq_kernel"), freq_stats)
        return out

    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, queries=args.queries)

    # ---- the memory-log segment
    t0 = time.perf_counter()
    cols, want = ref.memory_log(args.log_rows, args.locations, seed=1)
    rng = np.random.default_rng(9)
    rows_t = 1 << args.log_table
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
    d_table = to_dev(table)
    torch.cuda.synchronize()
    cap = (want.shape[1] - 1).bit_length()
    result["memory_log"] = dict(log_rows=args.log_rows, accesses=(1 << args.log_rows) - 5, fetches=1 << args.log_rows, program_rows=rows_t,
                                **measure("memory_log", seg, d_table, args.log_table, 0x1000, 4, cap, {}))
    trace = sa.memory_boundary_trace(seg, cap)[0]
    assert (om.from_monty(trace.cpu().numpy().view(np.uint32)).reshape(want.shape) == want).all()
    # the same fetches with the loop body at row 5000: its rows lie past the LDS partition
    if rows_t >= 8192:
        pick[: 1 << (args.log_rows - 1)] += 5000
        traces[1] = None
        traces[1] = to_dev(np.concatenate([table[:, pick], np.ones((1, 1 << args.log_rows), np.uint32)]))
        seg2 = [(provers[1], traces[1].data_ptr(), args.log_rows)]
        ts = []
        for it in range(args.warmup + args.steps):
            dt, r = timed(lambda: sa.program_frequencies(seg2, d_table, args.log_table, 0x1000, 4))
            assert r[1] == 0
            if it >= args.warmup:
                ts.append(dt)
        abi.lib.powdr_gpu_timing_enable(1)
        sa.program_frequencies(seg2, d_table, args.log_table, 0x1000, 4)
        torch.cuda.synchronize()
        fk = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in abi.timing_report().items()}.get("program_freq_kernel")
        abi.lib.powdr_gpu_timing_enable(0)
        result["memory_log"]["program_frequencies_loop_body_past_the_lds_partition"] = dict(stats(ts), program_freq_kernel=freq_rates(fk, sa.last_stats()))
    for p in provers:
        p.close()
    del traces, trace
    torch.cuda.empty_cache()

    # ---- the chained segment: records -> instruction AIRs on the device (the existing trace generation) -> the generators
    t0 = time.perf_counter()
    ex = vm.Execution(args.calls, seed=1)
    note("chained execution of", args.calls, "calls on the host in", round(time.perf_counter() - t0, 1), "s")
    itab = pc.InstructionTable(ex.block, [True] * len(ex.block), ex.start_pc)
    heights = pc.dummy_trace_heights(itab, ex.calls)
    d_rec = torch.from_numpy(np.ascontiguousarray(ex.rec).view(np.int32).reshape(-1)).cuda()
    bufs, seg, provers = [None] * pc.N_KINDS, [], []
    from powdr_amd import synth

    for k, h in enumerate(heights):
        if not h:
            continue
        t = torch.zeros(pc.WIDTHS[k] * h, dtype=torch.int32, device="cuda")
        bufs[k] = (t.data_ptr(), h)
        bc, sp, it = synth.reference_air_programs(ooc.KIND_NAMES[k])
        provers.append((prover.Prover(pc.WIDTHS[k], bc, sp, num_queries=args.queries, interactions=it), t))
        seg.append((provers[-1][0], t.data_ptr(), h.bit_length() - 1))
    expand = lambda: pc.expand(d_rec.data_ptr(), ex.calls, itab, bufs)
    expand()
    prog = sa.program_air(ex.program_table())
    result["chained"] = dict(calls=ex.calls, accesses=ex.accesses, instructions=len(ex.block),
                             **measure("chained", seg, prog.fixed_table(), prog.log_h, ex.start_pc, 4, 20, {"instruction_trace_generation": expand}))
    want = ref.boundary_trace(ex.initial, ex.final)
    trace = sa.memory_boundary_trace(seg, 20)[0]
    assert (om.from_monty(trace.cpu().numpy().view(np.uint32)).reshape(want.shape) == want).all()
    result["not_measured"] = ["a segment of 2^20 calls x 60 accesses = 2^26 accesses (the host-side construction of such a log is what limits the size here)",
                              "the interpreter path (POWDR_LOGUP_INTERPRET=1)", "peak scratch against a device budget",
                              "the kernels without their wave merging / LDS partition / load-before-atomic (no variant was built to compare)"]
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    for p, _ in provers:
        p.close()


if __name__ == "__main__":
    main()
