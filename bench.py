#!/usr/bin/env python3
"""bench.py — STARK cells/s (trace rows x main columns per second) of the MI355X proving path.

One "step" = one pass of the hot path over one segment's autoprecompile AIR:
    APC trace generation (gather + derived columns + bus->histogram replay, the three
    entry points of include/powdr_gpu.h, driven by the C++ host mirror
    powdr_apc_generate_witness_gpu) -> pw_prover_prove (iNTT, coset LDE, Poseidon2 Merkle
    commitments, quotient, openings, DEEP, FRI, queries) -> proof words on the host.
Inputs (the original chips' dummy traces, the periphery histograms) are resident in HBM when
the timed region starts. Workload at N=1: BASELINE.json configs[1] "guest-keccak autoprecompile
AIR, 2^20 rows" as the synthetic C2 shape of SURVEY.md §8d (W=2022, 187 constraints, 1734 bus
interactions, gathered from 5 original AIRs).

N>1: one process per GPU, every rank proves its own independent segments (weak scaling, no
data-path collective); the only RCCL traffic is the final all-gather of the per-segment trace
commitments (32 B per segment), inside the timed region.

Output: ONE JSON line on rank 0 (see the repository contract) — the COMPACT record (compact_line: under 6 000 bytes, strict JSON, every
string under 120 characters); the full record of the run (kernel tables, notes, every sub-benchmark) goes to bench_full.json (--full-out).

A plain run measures the headline only; --full adds every other leg and check (CPU baseline, the other proof kind, trace-generation
variants, multi_segment, C3, copy ceiling, live PMC). --dump-outputs DIR writes the last timed step's results as .npy files.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

P = 0x78000001
HBM_PEAK_GBS = 8000.0  # MI355X spec (MI355X_MICROARCH.md); ~6.3 TB/s achievable


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shape", default="C2")
    ap.add_argument("--log-height", type=int, default=None, help="override the trace height (default: the shape's)")
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--pow-bits", type=int, default=16)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-log-height", type=int, default=18,
                    help="rows (log2) of the CPU-baseline sample of the same AIR, minus one with the LogUp phase: 2^17 rows of C2 = 265 M cells, "
                         "~70 s on the box's host cores (round 5's 2^15-row sample under-stated the oracle ~2x: 256 OpenMP threads on 66 M cells; "
                         "cpu_baseline.full_size quotes the 2^20-row figure)")
    ap.add_argument("--no-logup-leg", "--no-second-leg", dest="no_logup_leg", action="store_true",
                    help="skip the second timed leg of the default run (the same step with the OTHER proof kind: `constraints_only`, or `logup` "
                         "under --constraints-only)")
    ap.add_argument("--no-callmajor-leg", action="store_true",
                    help="skip the measurement of the gather from call-major compacted sources (reported as `tracegen_callmajor`)")
    ap.add_argument("--logup-steps", "--second-steps", dest="logup_steps", type=int, default=3, help="timed steps of the second leg (after one warm-up step)")
    ap.add_argument("--no-live-pmc", action="store_true",
                    help="skip the two short rocprofv3 --pmc passes that measure the dominant kernel's HBM bytes and VALU instructions in this run")
    ap.add_argument("--no-copy-ceiling", action="store_true",
                    help="skip the 5 x 4 GiB device-to-device copies that measure the box's copy rate after the timed region "
                         "(they show up as __amd_rocclr_copyBuffer in rocprofv3 traces: 10.7 GB/step in the round-1 PMC pass)")
    ap.add_argument("--segments", type=int, default=8,
                    help="--shape C4 / C5 and the multi_segment leg: total number of independent segments, split over the ranks "
                         "by cell count (STRONG scaling: the total is fixed as N grows)")
    ap.add_argument("--segment-log-height", type=int, default=20, help="largest trace height (log2) of the C4 / C5 segment shapes")
    ap.add_argument("--no-segment-leg", action="store_true",
                    help="skip the multi_segment leg of the default run (C4: 10 APC AIRs + 19 system AIRs per segment, strong scaling)")
    ap.add_argument("--segment-steps", type=int, default=2, help="timed steps of the multi_segment leg (after one warm-up)")
    ap.add_argument("--segment-jit-all", action="store_true",
                    help="segment legs: compile EVERY AIR's specialised kernels once at set-up (pw_provers_specialise) instead of leaving it to the "
                         "library's per-proof rule (traces of >= 2^18 rows). Measured in round 6: C5 5.17 -> 5.41 G cells/s (the tail segment 170 -> "
                         "139 ms) for 145 s of cold compilation of its 61 AIRs; C4 6.67 -> 6.71 for 23 s: off by default")
    ap.add_argument("--segment-shapes", choices=("own", "equal"), default="own",
                    help="own: every segment has its OWN trace heights (HonestSegment.draw_shape: segment 0 at the caps, the last one a short tail, "
                         "the others one chip at its cap and the rest log-uniform over two octaves), like the reference's metered segments "
                         "(trace_generation.rs:113-131); equal: round 5's segments (same heights, other rows)")
    ap.add_argument("--segment-budget-frac", type=float, default=0.95,
                    help="the segment legs run under pw_set_device_budget(frac x the resident memory plan of the capped segment): the segment "
                         "whose AIRs are all at their caps crosses the streaming threshold (its largest AIRs are proven from coefficient arrays, "
                         "traces handed over), the others stay resident; 0 = no budget. profiles/r06_c4_budget_sweep.txt: 6.76 G cells/s without a "
                         "budget, 6.63 at 0.95 (one AIR of the capped segment on two sub-cosets), 6.36 at 0.8 (four AIRs of it, one of two more segments)")
    ap.add_argument("--no-c3-leg", action="store_true", help="skip the C3-scale leg of the default run (3 731 cols x 2^22 rows, reported as `c3`)")
    ap.add_argument("--pipeline", type=int, default=1,
                    help="host threads / HIP streams proving independent segments concurrently on each GPU "
                         "(throughput mode; default 1 = one segment at a time, which keeps per-kernel timings clean)")
    ap.add_argument("--constraints-only", action="store_true",
                    help="headline = the constraints-only proof (the AIR's bus interactions are replayed into the periphery histograms but are "
                         "not inside the proof); default: the proof includes them (pw-stark v0 + LogUp) — what PowdrAir::eval hands the "
                         "reference's backend (chip.rs:94-130) — and the constraints-only step is the `constraints_only` sub-record")
    ap.add_argument("--logup", action="store_true", help="(default since round 3; kept for old command lines)")
    ap.add_argument("--calls-fraction", type=float, default=1.0,
                    help="APC calls as a fraction of the trace height (SURVEY 8d asks for a 0.75 run: the rest is zero padding)")
    ap.add_argument("--inproc", action="store_true",
                    help="--shape C4 / C5 with --gpus N in ONE process: pw_prove_segments_multi (include/powdr_prover.h) — one host thread per "
                         "GPU behind the C ABI, RCCL all-gather of the commitments — instead of one torch.distributed rank per GPU")
    ap.add_argument("--launch-check", action="store_true",
                    help="start the ranks exactly as a real run would (self-launch under torch.distributed.run when --gpus N > 1 and no launcher "
                         "set WORLD_SIZE), let them meet over gloo on the CPU, print {launch_check, n_gpus, ranks} and exit: no GPU is touched")
    ap.add_argument("--exact-source-heights", action="store_true",
                    help="allocate dummy traces with b*calls rows instead of next_pow2 (less HBM)")
    ap.add_argument("--full-out", default=None,
                    help="where the full record of the run is written (default: bench_full.json next to this script; also POWDR_BENCH_FULL). "
                         "stdout carries the compact line only")
    ap.add_argument("--full", action="store_true",
                    help="also run everything the headline figure does not need: the CPU baseline, the second proof kind, the trace-generation "
                         "variants, the multi_segment and C3 legs, the copy ceiling, the live PMC passes and the segment checks (each one can "
                         "still be left out with its --no-* option). Without it a run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float64, rank 0): the proof "
                         "words, the periphery histograms and a fixed seeded sample of the trace (C2 / T shapes), or the merged "
                         "per-segment commitments (C4 / C5)")
    args = ap.parse_args()
    if not args.full:
        args.no_cpu_baseline = args.no_logup_leg = args.no_callmajor_leg = args.no_live_pmc = True
        args.no_copy_ceiling = args.no_segment_leg = args.no_c3_leg = True
    args.logup = not args.constraints_only
    global FULL_OUT
    FULL_OUT = args.full_out
    return args


_T0 = time.perf_counter()


def phase(name):
    """POWDR_BENCH_TRACE=1: wall-clock marks on stderr (where a run's seconds outside the timed regions go)."""
    if os.environ.get("POWDR_BENCH_TRACE"):
        print(f"[bench rank {os.environ.get('RANK', '0')} +{time.perf_counter() - _T0:7.2f}s] {name}", file=sys.stderr, flush=True)


LINE_LIMIT = 6000  # bytes; BENCH_r04.json.parsed was null on a 23 KB line
FULL_OUT = None    # --full-out / POWDR_BENCH_FULL; default <repo>/bench_full.json


def _clean(x, sig=6, strlen=None):
    """Strict-JSON value: non-finite floats -> None, floats to `sig` significant digits, numpy scalars -> python, strings cut to `strlen`."""
    import math

    if isinstance(x, dict):
        return {str(k): _clean(v, sig, strlen) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_clean(v, sig, strlen) for v in x]
    if isinstance(x, (bool, type(None))):
        return x
    if isinstance(x, (np.bool_,)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        x = float(x)
        if not math.isfinite(x):
            return None
        return float(f"{x:.{sig}g}") if sig else x
    if isinstance(x, str):
        return x if strlen is None or len(x) <= strlen else x[:strlen - 1] + "~"
    return str(x)


def _pick(d, *keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d} if isinstance(d, dict) else None


def compact_line(full: dict) -> dict:
    """The line the driver reads: the contract's fields plus ONE number (or a handful) per sub-benchmark; every string under 120 characters.
    Everything else — kernel tables, notes, per-kernel rooflines, the trace-generation variants — lives in bench_full.json."""
    if full.get("launch_check"):
        return _clean(full)
    out = _pick(full, "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "rccl_ranks", "per_rank_ms", "strong_scaling_value")
    out["metric"] = full.get("metric_short") or out.get("metric")
    cfg = full.get("config") or {}
    out["config"] = _pick(cfg, "rows", "cols", "perm_cols", "proof_bytes", "parallelism")
    out["config"] = dict(workload=cfg.get("workload_short") or cfg.get("workload"), **out["config"])
    r = full.get("roofline")
    if r:
        rr = _pick(r, "bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_step", "avg_launch_ms", "launches_per_step")
        if r.get("whole_step"):
            rr["whole_step"] = _pick(r["whole_step"], "frac", "achieved_GBps", "algo_bytes_per_cell")
        if r.get("valu"):
            rr["valu"] = _pick(r["valu"], "frac", "valu_instr_per_perm")
        out["roofline"] = rr
    else:
        out["roofline"] = None
    c = full.get("cpu_baseline")
    if c:
        cc = _pick(c, "value", "unit", "cores", "kind", "sample")
        cc["sample"] = c.get("sample_short") or cc.get("sample")
        if c.get("tuned"):
            cc["tuned"] = _pick(c["tuned"], "value", "upper_bound_commit_stages_only")
        if c.get("full_size"):
            cc["full_size"] = _pick(c["full_size"], "value", "value_prover_only", "cores", "log_height", "source")
        out["cpu_baseline"] = cc
    else:
        out["cpu_baseline"] = None
    for key in ("constraints_only", "logup"):
        if full.get(key):
            out[key] = _pick(full[key], "value", "ms_per_step", "error")
    c3 = full.get("c3")
    if c3:
        out["c3"] = _pick(c3, "value", "prove_ms", "trace_gen_ms", "verify_rc", "logup", "cells", "committed_columns", "stream_log_blocks", "trace_handed_over",
                          "specialise_s", "skipped", "error")
        if isinstance(c3.get("segment"), dict):
            out["c3"]["segment"] = _pick(c3["segment"], "prove_ms", "verify_rc", "apc_air_stream_log_blocks", "trace_handed_over", "error")
    ms = full.get("multi_segment")
    if ms:
        m = _pick(ms, "value", "ms_per_step", "verify_rc", "n_segments", "distinct_segments", "constraint_violations", "segment_shapes", "cells_by_segment",
                  "device_budget_bytes", "error")
        if isinstance(ms.get("streamed_airs_by_segment"), dict):
            m["segments_with_streamed_airs"] = sorted(int(u) for u, v in ms["streamed_airs_by_segment"].items() if v)
        if isinstance(ms.get("lookup_balance"), dict):
            m["lookup_balance_rc"] = ms["lookup_balance"].get("verify_rc")
        out["multi_segment"] = m
    tr = (full.get("tracegen_from_records") or {}).get("timed_step")
    if tr:
        out["tracegen_from_records"] = dict(timed_step=_pick(tr, "ms_per_step", "value", "error"))
    if full.get("stage_ms"):
        out["stage_ms"] = {k: v for k, v in full["stage_ms"].items()}
    if full.get("gauges"):
        out["gauges"] = {k: v for k, v in full["gauges"].items() if k != "note"}
    if full.get("comm"):
        out["comm"] = _pick(full["comm"], "backend", "launch", "ranks")
    if full.get("jit_cache"):
        out["jit_cache"] = dict(units_compiled=sum(full["jit_cache"]["units_compiled"]), units_from_disk=sum(full["jit_cache"]["units_from_disk"]))
    out["hbm_copy_GBps_measured"] = full.get("hbm_copy_GBps_measured")
    out["full_record"] = full.get("full_record")
    out = _clean(out, sig=6, strlen=119)
    # belt and braces: never above the limit, whatever a future sub-record adds
    for victim in ("gauges", "stage_ms", "tracegen_from_records", "comm", "per_rank_ms"):
        if len(json.dumps(out, allow_nan=False, separators=(", ", ": "))) <= LINE_LIMIT:
            break
        if victim == "stage_ms" and isinstance(out.get("stage_ms"), dict):  # keep the five largest first
            top = sorted(out["stage_ms"].items(), key=lambda kv: -(kv[1] or 0))[:5]
            out["stage_ms"] = dict(top)
            continue
        out.pop(victim, None)
    if len(json.dumps(out, allow_nan=False, separators=(", ", ": "))) > LINE_LIMIT:
        # still too long after every optional block went: the contract's fields and the pointer to the full record, nothing else
        print("bench.py: compact record above the line limit; printing the contract fields only", file=sys.stderr)
        keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline", "full_record")
        out = {k: out.get(k) for k in keep if k in out}
        for victim in ("cpu_baseline", "roofline", "config"):
            if len(json.dumps(out, allow_nan=False, separators=(", ", ": "))) <= LINE_LIMIT:
                break
            v = out.get(victim)
            out[victim] = {k: x for k, x in v.items() if not isinstance(x, (dict, list, str)) or k in ("bound", "unit", "kind", "workload")} if isinstance(v, dict) else None
    return out


def emit(line: dict):
    """The ONE JSON line, as the last thing on stdout: RCCL writes a version banner through C stdio when a communicator is created
    (torch.distributed's nccl backend, pw_prove_segments_multi) and a pipe buffers it until exit, i.e. until after our line.
    The line is the COMPACT record (compact_line: <= LINE_LIMIT bytes, strict JSON); the full record of the run goes to bench_full.json
    next to this script (--full-out / POWDR_BENCH_FULL name another place). Nothing large goes to stderr: the driver's tail holds both."""
    import ctypes

    full_path = Path(FULL_OUT or os.environ.get("POWDR_BENCH_FULL") or ROOT / "bench_full.json")
    if not line.get("launch_check"):
        try:
            full_path.parent.mkdir(parents=True, exist_ok=True)
            full_path.write_text(json.dumps(_clean(line, sig=0), allow_nan=False, indent=1) + "\n")
            line = dict(line, full_record=str(full_path.relative_to(ROOT)) if full_path.is_relative_to(ROOT) else str(full_path))
        except OSError as e:
            print(f"bench.py: could not write {full_path}: {e}", file=sys.stderr)
    text = json.dumps(compact_line(line), allow_nan=False)
    if len(text) > LINE_LIMIT:  # (compact_line degrades to the contract's fields; a line is printed whatever happens)
        print(f"bench.py: line of {len(text)} bytes is above the {LINE_LIMIT}-byte limit", file=sys.stderr)
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()
    print(text, flush=True)


def self_launch(args):
    """`python bench.py --gpus N` (N > 1) as typed, with no launcher around it: become the launcher. Re-runs this command as N ranks
    under torch.distributed.run — the form the driver uses (`-m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr
    127.0.0.1 --master-port P bench.py ...`) — and passes their output and exit code through. A run that was asked for N GPUs never
    silently measures one."""
    import socket
    import subprocess

    if args.gpus <= 1 or "WORLD_SIZE" in os.environ or args.inproc:
        return
    env = dict(os.environ, POWDR_BENCH_LAUNCH="self")
    if not args.launch_check and env.get("POWDR_DIST_BACKEND", "nccl") == "nccl" and torch.cuda.device_count() < args.gpus:
        print(f"bench.py: --gpus {args.gpus} but only {torch.cuda.device_count()} device(s) are visible; an N-GPU line is not produced on fewer "
              f"GPUs (POWDR_DIST_BACKEND=gloo runs all ranks on GPU 0: the test hook of one-GPU boxes)", file=sys.stderr)
        sys.exit(2)
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve())] + sys.argv[1:]
    sys.stdout.flush()
    sys.exit(subprocess.call(cmd, env=env))


def launch_check():
    """--launch-check: the ranks meet over gloo on the CPU and rank 0 reports who is there."""
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    ranks = [0]
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
        got = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(got, torch.tensor([rank], dtype=torch.int64))
        ranks = [int(t.item()) for t in got]
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        emit(dict(launch_check=True, n_gpus=world, ranks=ranks, launch=os.environ.get("POWDR_BENCH_LAUNCH", "external" if world > 1 else "single process")))


def setup_distributed(n):
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # test hook: POWDR_DIST_BACKEND=gloo runs the N>1 code path with every rank on GPU 0 (one-GPU boxes)
        backend = os.environ.get("POWDR_DIST_BACKEND", "nccl")
        if backend == "nccl":
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            torch.cuda.set_device(0)
            dist.init_process_group(backend)
    else:
        torch.cuda.set_device(0)
    return rank, local, world


def build_workload(shape_name, log_h, exact_heights, seed, calls_fraction=1.0, data_seed=None):
    """One APC AIR's trace-generation inputs, resident in HBM (powdr_amd/segment_workload.py build_apc_workload)."""
    from powdr_amd import segment_workload as sw

    return sw.build_apc_workload(shape_name, log_h, exact_heights, seed, calls_fraction, data_seed=data_seed)


def cpu_baseline(shape_name, log_h, queries, pow_bits, seed, logup=False):
    """The CPU oracle (a restatement, kind 'port') on a bounded sample of the same workload:
    the reference's CPU trace generation (row-major, sequential row loop) + the pw-stark v0 oracle
    prover, on this box's host cores."""
    from oracle import apc_model as om
    from oracle import stark_model as sm
    from powdr_amd import synth

    s = synth.generate(shape_name, seed=seed)
    apc = om.load_apc(s.doc)
    idx = apc.poly_id_to_index()
    calls = 1 << log_h
    bufs, dims = synth.fill_dummy_traces_numpy(s, calls, seed)
    ct = om.build_cpu_tables(apc, idx)
    name_to = {n: i for i, (n, _, _, _) in enumerate(dims)}
    dummy_rm, dummy_w = [], []
    for n in ct.air_names:
        _, w, h, b = dims[name_to[n]]
        dummy_rm.append(np.ascontiguousarray(bufs[name_to[n]].reshape(w, h).T))
        dummy_w.append(w)
    per = dict(var_bus=3, var_hist=np.zeros(1 << 18, np.uint32), tuple_bus=7, tuple_hist=np.zeros(256 * 2048, np.uint32),
               sz0=256, sz1=2048, bitwise_bus=6, bitwise_hist=np.zeros(2 * 65536, np.uint32))
    bc, spans = sm.compile_constraints(apc, idx)
    om.c_oracle()
    t0 = time.perf_counter()
    vals = om.c_generate_witness(apc, ct, idx, dummy_rm, dummy_w, calls, per)
    t1 = time.perf_counter()
    flat = np.ascontiguousarray(vals.T).reshape(-1)
    if logup:
        it = sm.compile_interactions(apc, idx)
        proof = sm.prove_logup(flat, len(idx), log_h, bc, spans, *it, num_queries=queries, pow_bits=min(pow_bits, 12))
    else:
        proof = sm.prove(flat, len(idx), log_h, bc, spans, num_queries=queries, pow_bits=min(pow_bits, 12))
    t2 = time.perf_counter()
    cells = len(idx) * calls
    cores = os.cpu_count() or 1
    tuned = None
    try:
        tuned = cpu_baseline_tuned(len(idx), (4 * len(sm.group_starts(*it)) if logup else 0) + 8, log_h, cells, t1 - t0, t2 - t1, cores)
    except Exception as e:  # the tuned figure is an extra
        tuned = dict(value=None, error=f"{type(e).__name__}: {e}")
    full_size = cpu_baseline_full_size(shape_name, len(idx), logup, log_h, t1 - t0)
    return dict(value=cells / (t2 - t0), unit="cells/s", cores=cores, kind="port", tuned=tuned, full_size=full_size,
                sample=f"{shape_name} AIR W={len(idx)} at 2^{log_h} rows ({cells} cells): oracle trace generation "
                       f"(single thread, like the reference's row loop) {t1 - t0:.2f}s + oracle prover{' with the LogUp phase' if logup else ''} "
                       f"(OpenMP, {cores} threads) {t2 - t1:.2f}s",
                sample_short=f"{shape_name} W={len(idx)} at 2^{log_h} rows ({cells / 1e6:.1f} M cells): oracle tracegen 1 thread {t1 - t0:.1f} s + oracle "
                             f"prover{' +LogUp' if logup else ''} OpenMP x{cores} {t2 - t1:.1f} s",
                trace_gen_s=t1 - t0, prove_s=t2 - t1)


def cpu_baseline_full_size(shape_name, width, logup, sample_log_h, sample_trace_gen_s):
    """The same oracle at the FULL size of the GPU workload, from the committed profile of the run that byte-compared the two proofs
    (tools/full_size_parity.py: the oracle prover on all host cores of a GPU box of this pool, 2^20 rows) — too long for every bench run
    (~8 minutes), so it is quoted, with its file; trace generation (the reference's sequential row loop, cpu/mod.rs:161-225: exactly
    linear in the rows) is this run's own single-thread sample scaled to the full height. The live `value` above is a SAMPLE of the
    same code; VERDICT r5 #3: it has to land within 25 % of this figure."""
    name = {("C2", True): "r03_full_size_parity_c2_logup.json", ("C2", False): "r02_full_size_parity_c2.json"}.get((shape_name, bool(logup)))
    f = ROOT / "profiles" / name if name else None
    if f is None or not f.exists():
        return None
    try:
        d = json.loads(f.read_text())
        if d.get("cols") != width or not d.get("proofs_identical"):
            return None
        rows = 1 << d["log_height"]
        tg = sample_trace_gen_s * rows / (1 << sample_log_h)
        cells = width * rows
        return dict(value=cells / (tg + d["oracle_prove_s"]), value_prover_only=cells / d["oracle_prove_s"], unit="cells/s", cores=d.get("host_cores"),
                    log_height=d["log_height"], prove_s=d["oracle_prove_s"], trace_gen_s_scaled_from_sample=tg, source=f"profiles/{name}",
                    note="oracle prover at the GPU workload's full size (committed profile, proof words identical to the HIP prover's) + this run's "
                         "single-thread trace generation scaled linearly to that height")
    except Exception as e:  # a quoted figure must never cost the line
        return dict(value=None, error=f"{type(e).__name__}: {e}")


def cpu_baseline_tuned(width, extra_cols, log_h, cells, oracle_tracegen_s, oracle_prove_s, cores):
    """What a TUNED CPU prover could plausibly reach on this box: the two stages that dominate the proof — LDE
    and Poseidon2 Merkle commitment of every committed column (main trace + LogUp permutation matrix + quotient chunks) — are
    re-timed with oracle/tuned_cpu.cpp (Montgomery arithmetic, AVX-512, lane = column / lane = row like Plonky3's row-major
    kernels; results equal to the oracle's, tests/test_tuned_cpu.py) and with the naive oracle on the same random matrix; the
    remaining stages keep the oracle's time: tuned prove = oracle prove - naive (LDE + Merkle) + tuned (LDE + Merkle)."""
    import ctypes as C

    from oracle import apc_model as om
    from oracle import stark_model as sm

    lib = om.tuned_cpu()
    p_ = lambda a: a.ctypes.data_as(C.c_void_p)
    cols, H = width + extra_cols, 1 << log_h
    m = np.random.default_rng(1).integers(0, P, cols * H, dtype=np.uint32)
    lde = np.zeros(cols * 2 * H, np.uint32)
    root = np.zeros(8, np.uint32)
    lib.tc_lde(p_(m[: 16 * H]), C.c_uint32(16), C.c_int(log_h), p_(lde))  # warm-up (threads, tables)
    t0 = time.perf_counter()
    lib.tc_lde(p_(m), C.c_uint32(cols), C.c_int(log_h), p_(lde))
    t1 = time.perf_counter()
    lib.tc_merkle_root(p_(lde), C.c_size_t(2 * H), C.c_uint32(cols), p_(root))
    t2 = time.perf_counter()
    want = sm.lde(m, cols, log_h)
    t3 = time.perf_counter()
    oroot = sm.merkle_commit(want, 2 * H, cols)
    t4 = time.perf_counter()
    same = bool((want == lde).all() and (np.asarray(oroot).reshape(-1)[:8] == root).all())
    tuned_prove = max(oracle_prove_s - (t4 - t2), 0.0) + (t2 - t0)
    return dict(value=cells / (oracle_tracegen_s + tuned_prove), value_prover_only=cells / tuned_prove,
                upper_bound_commit_stages_only=cells / (t2 - t0), unit="cells/s", cores=cores, kind="tuned-stages",
                avx512=bool(lib.tc_has_avx512()), committed_columns=cols, tuned_lde_s=t1 - t0, tuned_merkle_s=t2 - t1, naive_lde_s=t3 - t2,
                naive_merkle_s=t4 - t3, other_stages_s=max(oracle_prove_s - (t4 - t2), 0.0), equals_oracle=same,
                note="LDE + Poseidon2 Merkle of all committed columns with Montgomery/AVX-512 kernels (oracle/tuned_cpu.cpp), the remaining stages "
                     "(quotient, permutation trace, openings, FRI) at the naive oracle's speed, trace generation single-threaded like the reference's "
                     "row loop (cpu/mod.rs:161-225); value_prover_only leaves trace generation out; upper_bound_commit_stages_only = main cells / "
                     "(tuned LDE + tuned Merkle) alone — what a CPU prover whose every other stage were free would reach on these cores, i.e. the "
                     "GPU figure divided by it is a LOWER bound of the speed-up over any CPU prover built from kernels of this quality")


ALGO_BYTES_PER_CELL = 48.0  # tracegen 8 + LDE 12 + Merkle 8 + quotient 8 + DEEP/openings 12 (whole pipeline, per main cell)


def timed_leg(run_steps, steps, warmup, barrier, abi, world):
    """W untimed steps, then exactly K steps between barrier + synchronize; max over ranks; per-kernel event timing."""
    run_steps(warmup)
    barrier()
    abi.lib.powdr_gpu_timing_enable(1)
    t0 = time.perf_counter()
    run_steps(steps)
    barrier()
    t1 = time.perf_counter()
    timing = abi.timing_report()
    abi.lib.powdr_gpu_timing_enable(0)
    elapsed = t1 - t0
    LAST_PER_RANK_S[:] = [elapsed]
    if world > 1:
        import torch.distributed as dist

        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        mine = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        every = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
        dist.all_gather(every, mine)
        LAST_PER_RANK_S[:] = [float(t.item()) for t in every]
        elapsed = max(LAST_PER_RANK_S)  # the contract: max over ranks
    return elapsed, timing


LAST_PER_RANK_S = [0.0]  # seconds of the last timed_leg on every rank (rank order)


def comm_facts(world):
    """Who took part, as the communicator itself reports it (not as the command line asked)."""
    if world <= 1:
        return dict(ranks=1, backend=None, launch=os.environ.get("POWDR_BENCH_LAUNCH", "single process"))
    import torch.distributed as dist

    backend = dist.get_backend()
    return dict(ranks=dist.get_world_size(), backend=("RCCL (torch.distributed nccl)" if backend == "nccl" else backend),
                launch=os.environ.get("POWDR_BENCH_LAUNCH", "external launcher (torch.distributed.run)"),
                devices_visible=torch.cuda.device_count(),
                note=None if backend == "nccl" else "POWDR_DIST_BACKEND test hook: every rank on GPU 0, collectives over gloo - not a multi-GPU measurement")


def jit_cache_by_rank(world):
    """Translation units every rank compiled / loaded from the shared on-disk cache (pw_jit_cache_stats), gathered on all ranks: with
    N ranks specialising the same AIRs the compile phase is serialised by the cache directory's lock, so every unit is compiled by
    exactly one of them. Collective: every rank calls it."""
    from powdr_amd import prover

    st = prover.jit_cache_stats()
    mine = [int(st["compiled"]), int(st["from_disk"])]
    if world <= 1:
        return dict(units_compiled=[mine[0]], units_from_disk=[mine[1]])
    import torch.distributed as dist

    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    got = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(got, torch.tensor(mine, dtype=torch.int64, device=dev))
    return dict(units_compiled=[int(t[0]) for t in got], units_from_disk=[int(t[1]) for t in got])


def gauges_of(stage_ms):
    """Kernel times grouped under the reference's gauge names (openvm/metrics-viewer/CLAUDE.md:55-116)."""
    g = lambda *names: sum(stage_ms.get(n, 0.0) for n in names)
    return dict(
        trace_gen_time_ms=g("apc_gather_tile_kernel", "apc_apply_derived_expr_kernel", "apc_apply_bus_kernel", "bus_histogram_kernel"),
        main_trace_commit_time_ms=g("ntt_group_kernel<dif>", "lde_fused_kernel", "ntt_group_kernel<dit>", "leaf_hash_kernel", "compress_kernel", "compress_tail_kernel"),
        perm_trace_time_ms=g("logup_perm_kernel", "logup_perm_jit_kernel", "logup_rowsum_combine_kernel", "logup_scan_kernels"),
        quotient_poly_compute_time_ms=g("quotient_kernel", "quotient_jit_kernel", "quotient_combine_kernel", "quotient_logup_kernel", "quotient_logup_jit_kernel",
                                        "quotient_logup_tail_kernel", "quotient_split_kernel"),
        pcs_opening_time_ms=g("barycentric_weights_kernel", "zeta_weights_kernel", "ext_dot_partial_kernel", "deep_kernel", "deep_logup_kernel",
                              "ext_pair_leaf_kernel", "fri_fold_kernel", "gather_rows_kernel"),
        note="main_trace_commit also contains the 8-column quotient commitment (and, with LogUp, the permutation matrix's; same kernels); "
             "stark_prove_excluding_trace_time_ms = ms_per_step - trace_gen_time_ms")


def _segment_checks(seg, segments, rec, distinct=True, shapes=None):
    """After the timed region, for EVERY segment in `segments` (the ones this process proved; their inputs are staged again one at a time):
    the proof against the product's host verifier, the device's mock prover on the traces it was made from, and the lookup buses'
    balance (segment_workload.HonestSegment.balance_witness). Into `rec`: the worst code over the segments + the per-segment lists."""
    t0 = time.perf_counter()
    vrc, viol, roots = [], [], []
    hdr = 5 + 4 * len(seg.airs)
    stage = (lambda u: seg.stage_inputs(u, shapes[u])) if shapes is not None else seg.stage_inputs
    for u in segments:
        if distinct:
            stage(u)
        seg.generate_traces()
        pf = np.array(seg.prove(), copy=True)
        vrc.append(int(seg.verify(pf)))
        viol.append(int(seg.check_constraints()))
        roots.append(tuple(int(x) for x in pf[hdr:hdr + 8]))
    rec["verify_rc"] = max(vrc, key=abs) if vrc else None
    rec["verify_rc_by_segment"] = vrc
    rec["verify_s"] = time.perf_counter() - t0
    rec["constraint_violations"] = int(sum(viol))
    rec["checked_segments"] = [int(u) for u in segments]
    rec["distinct_commitments"] = len(set(roots))
    prev = os.environ.get("POWDR_JIT")
    try:
        os.environ["POWDR_JIT"] = "0"  # the witness is proven once per segment: not worth compiling 26 more sets of kernels
        seg.release_provers()
        brc, totals = [], []
        for u in segments:
            if distinct:
                stage(u)
            seg.generate_traces()
            rc, total = seg.balance_witness()
            brc.append(int(rc))
            totals.append([int(x) for x in total])
        rec["lookup_balance"] = dict(verify_rc=max(brc, key=abs) if brc else None, verify_rc_by_segment=brc,
                                     total_sum=[max(t[k] for t in totals) for k in range(4)] if totals else None, buses=[3, 6, 7],
                                     note="per segment: the same traces, every AIR restricted to the lookup buses (var-range 3, bitwise 6, tuple 7), one segment "
                                          "proof, pw_verify_segment with check_balance: the APC and instruction AIRs' sends and the periphery AIRs' receives cancel "
                                          "(total_sum: the largest word over the segments). Memory / execution-bridge / program buses: send side only (their "
                                          "receivers are external chips)")
    except Exception as e:
        rec["lookup_balance"] = dict(verify_rc=None, error=f"{type(e).__name__}: {e}")
    finally:
        if prev is None:
            os.environ.pop("POWDR_JIT", None)
        else:
            os.environ["POWDR_JIT"] = prev


SPECIALISE_ALL = False  # --segment-jit-all: the segment legs compile every AIR's specialised kernels at set-up
SEGMENT_SHAPES, SEGMENT_BUDGET_FRAC = "own", 0.95  # (--segment-shapes / --segment-budget-frac; set in main)


def _segment_plan(seg, n_segments):
    """(shapes, cells, log-heights) per segment: the segments' own trace heights (--segment-shapes own) or the caps for all."""
    shapes = [seg.draw_shape(u, n_segments) if SEGMENT_SHAPES == "own" else None for u in range(n_segments)]
    return shapes, [int(seg.shape_cells(sh)) for sh in shapes], [seg.shape_heights(sh) for sh in shapes]


def _segment_budget(seg, shapes, prover):
    """The capped segment (every AIR at its cap) proven once, outside any timed region, to read its resident memory plan; the budget
    the leg then runs under is SEGMENT_BUDGET_FRAC of it (an embedder sharing the device would set such a budget). Returns the record."""
    if not SEGMENT_BUDGET_FRAC or SEGMENT_SHAPES != "own":
        return dict(device_budget_bytes=None)
    seg.stage_inputs(0, None)
    seg.generate_traces()
    seg.prove()
    resident = prover.segment_last_plan()[0]
    budget = int(SEGMENT_BUDGET_FRAC * resident)
    prover.set_device_budget(budget)
    return dict(device_budget_bytes=budget, resident_plan_bytes_capped_segment=int(resident), budget_frac=SEGMENT_BUDGET_FRAC)


def _shape_record(seg, shapes, cells, heights):
    names = [a["name"] for a in seg.airs]
    return dict(segment_shapes=SEGMENT_SHAPES, air_names=names, heights_by_segment=heights, cells_by_segment=cells,
                calls_by_segment=[None if sh is None else dict(apc=sh["apc_calls"], instruction_block=sh["instr_calls"]) for sh in shapes],
                shape_note="per segment its own trace heights, like a metered execution's (trace_generation.rs:113-131): segment 0 every chip at its cap, "
                           "the last one the execution's tail (<= 1/8), the others one chip at its cap and the rest log-uniform over two octaves; "
                           "log2 heights in air_names order" if SEGMENT_SHAPES == "own" else "every segment at the caps (round 5's legs)")


def segment_bench_inproc(kind, n_segments, max_log_height, steps, warmup, logup, queries, pow_bits, n_workers, abi, checks=True):
    """The same strong-scaling workload as segment_bench, driven from ONE process through the C ABI's multi-device entry
    pw_prove_segments_multi: one host thread per worker (worker w on GPU w mod #GPUs) with its own launch stream and its own
    replica of the segment (trace generators, provers, buffers); placement by cells; the only exchange is the RCCL all-gather of
    the 8-word commitments at the end of every step."""
    from powdr_amd import prover, segment_workload as sw

    n_dev = torch.cuda.device_count()
    devices = [w % n_dev for w in range(n_workers)]
    workers = []
    for w in range(n_workers):
        with torch.cuda.device(devices[w]):
            workers.append(sw.HonestSegment(kind, max_log_height=max_log_height, seed=0, queries=queries, pow_bits=pow_bits, logup=logup,
                                            specialise_all=SPECIALISE_ALL))
    for d in set(devices):
        torch.cuda.synchronize(d)
    seg0 = workers[0]
    shapes, cells, heights = _segment_plan(seg0, n_segments)
    hdr = 5 + 4 * len(seg0.airs)
    last = {}
    with torch.cuda.device(devices[0]):
        budget = _segment_budget(seg0, shapes, prover)

    mine0 = set()
    streamed = {}

    def prove_one(segment, worker, device):
        # every segment has its own inputs AND its own trace heights, staged in the worker's buffers; the traces are handed over
        workers[worker].stage_inputs(segment, shapes[segment])
        workers[worker].generate_traces()
        pf = workers[worker].prove(hand_over=True)
        streamed[int(segment)] = [f"{a['name']}:{1 << b} sub-cosets" for a, (b, _) in zip(workers[worker].airs, prover.segment_last_modes()) if b]
        last["words"] = len(pf)
        if worker == 0:
            mine0.add(int(segment))
        return pf[hdr:hdr + 8].copy()

    def run_steps(n):
        for _ in range(n):
            last["merged"], last["owner"], last["merge"] = prover.prove_segments_multi(devices, cells, prove_one)

    def barrier():
        for d in set(devices):
            torch.cuda.synchronize(d)

    run_steps(warmup)
    barrier()
    t0 = time.perf_counter()
    run_steps(steps)
    barrier()
    elapsed = time.perf_counter() - t0
    assert (last["merged"] != 0).any(axis=1).all(), "a segment's commitment is missing from the merge"
    rec = dict(shape=kind, scaling="strong", n_segments=n_segments, workers=n_workers, devices=devices, airs_per_segment=len(seg0.airs),
               cells_per_segment=max(cells), cells_per_step=sum(cells), value=sum(cells) * steps / elapsed, unit="cells/s", ms_per_step=elapsed / steps * 1e3,
               steps=steps, warmup=warmup, logup=bool(logup), proof_bytes_per_segment=int(last["words"]) * 4,
               segments_per_worker=[int((last["owner"] == w).sum()) for w in range(n_workers)],
               cells_per_worker=[int(sum(c for c, o in zip(cells, last["owner"]) if o == w)) for w in range(n_workers)],
               streamed_airs_by_segment=[streamed.get(u, []) for u in range(n_segments)], traces_handed_over=True, **budget,
               **_shape_record(seg0, shapes, cells, heights),
               commitment_merge={1: "RCCL all-gather (one communicator per device set, ncclCommInitAll at first use)", 2: "host (RCCL not available)"}[last["merge"]],
               note="pw_prove_segments_multi: one process, one host thread + launch stream per worker; per segment: trace generation of every AIR + one "
                    "pw-stark v1 proof (segment_workload.HonestSegment: one resident segment per worker, regenerated and proven for every unit)")
    rec["distinct_segments"] = True
    LAST_OUTPUTS["segment_commitments"] = np.array(last["merged"], copy=True)
    prover.set_device_budget(0)
    if checks:
        with torch.cuda.device(devices[0]):
            _segment_checks(seg0, sorted(mine0), rec, shapes=shapes)
    for wk in workers:
        wk.close()
    return rec


def segment_bench(kind, n_segments, max_log_height, steps, warmup, logup, queries, pow_bits, rank, world, abi, barrier, checks=True):
    """Multi-AIR segments, STRONG scaling: a fixed number of independent segments is placed on the
    ranks by cell count; every rank handles its segments one after the other — trace generation of EVERY AIR of the segment (APC
    AIRs: gather + derived columns + bus replay; instruction AIRs: record expansion + replay of their lookups; periphery AIRs from
    the histograms) and ONE pw-stark v1 proof (pw_prove_segment: all AIRs of a phase in one mixed-height commitment, one FRI), both
    inside the timed region — and the main commitments are all-gathered (32 B per segment). Every rank keeps ONE resident segment
    (powdr_amd/segment_workload.py) whose INPUTS are replaced per unit by those of the segment being proven (HonestSegment.stage_inputs:
    a real execution's segments differ in values, not in shape). After the timed region: host verification, the device's mock prover
    and the lookup buses' balance for every segment rank 0 proved. Returns the record (rank 0) or None."""
    from powdr_amd import segment_workload as sw, sharding

    from powdr_amd import prover

    t_spec = time.perf_counter()
    seg = sw.HonestSegment(kind, max_log_height=max_log_height, seed=0, queries=queries, pow_bits=pow_bits, logup=logup,
                           specialise_all=SPECIALISE_ALL)
    t_spec = time.perf_counter() - t_spec
    shapes, cells, heights = _segment_plan(seg, n_segments)
    hdr = 5 + 4 * len(seg.airs)  # proof words before the main commitment
    last = dict(gen_s=0.0, prove_s=0.0, stage_s=0.0, units=0)
    budget = _segment_budget(seg, shapes, prover)
    streamed, unit_ms = {}, {}

    def prove_one(u):
        # segment u's OWN inputs (the dummy traces behind every APC AIR, the instruction AIRs' records), generated on the device into the
        # resident segment's buffers: inside the timed region (one write-only pass over the sources, reported as input_staging_ms_per_segment)
        ts = time.perf_counter()
        seg.stage_inputs(u, shapes[u])  # ... at the segment's OWN trace heights (re-planning, buffer reuse and kernel-cache hits inside the timed region)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seg.generate_traces()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        pf = seg.prove(hand_over=True)  # every chip moves its trace into the engine (cuda/mod.rs:415-419)
        t2 = time.perf_counter()
        streamed[int(u)] = [f"{a['name']}:{1 << b} sub-cosets" for a, (b, _) in zip(seg.airs, prover.segment_last_modes()) if b]
        unit_ms[int(u)] = dict(stage=(t0 - ts) * 1e3, trace_gen=(t1 - t0) * 1e3, prove=(t2 - t1) * 1e3)
        last["stage_s"] += t0 - ts
        last["gen_s"] += t1 - t0
        last["prove_s"] += t2 - t1
        last["units"] += 1
        last["words"] = len(pf)
        return pf[hdr:hdr + 8].copy()

    def run_steps(n):
        for _ in range(n):
            mine, merged = sharding.prove_segments_sharded(cells, prove_one, rank, world)
            last["mine"], last["merged"] = mine, merged

    run_steps(warmup)
    last.update(gen_s=0.0, prove_s=0.0, stage_s=0.0, units=0)
    elapsed, timing = timed_leg(run_steps, steps, 0, barrier, abi, world)
    per_rank_ms = [t / steps * 1e3 for t in LAST_PER_RANK_S]
    assert (last["merged"] != 0).any(axis=1).all(), "a segment's commitment is missing from the merge"
    total_cells = sum(cells) * steps
    stage = {k: ms / steps for k, (c, ms) in timing.items()}
    units = max(1, last["units"])
    cells_mine = sum(cells[u] for u in last["mine"]) or 1
    cap_heights = seg.shape_heights(None)
    air_shapes = [(a["name"], a["width"], lh, len(a["cons"][1]), len(a["inter"][0])) for a, lh in zip(seg.airs, cap_heights)]
    placement = sharding.assign_units(list(cells), world)
    rec = dict(shape=kind, scaling="strong", n_segments=n_segments, segments_on_rank0=len(last["mine"]), airs_per_segment=len(air_shapes),
               airs_by_role={r: sum(1 for a in seg.airs if a["role"] == r) for r in ("apc", "instruction", "periphery")},
               cells_per_segment=int(seg.shape_cells(None)), cells_per_step=sum(cells), value=total_cells / elapsed, unit="cells/s", ms_per_step=elapsed / steps * 1e3, steps=steps,
               placement=[[int(u) for u in p_] for p_ in placement], cells_per_rank=[int(sum(cells[u] for u in p_)) for p_ in placement],
               streamed_airs_by_segment={str(u): v for u, v in sorted(streamed.items())}, ms_by_segment_rank0={str(u): v for u, v in sorted(unit_ms.items())},
               traces_handed_over=True, **budget, **_shape_record(seg, shapes, cells, heights),
               airs_specialised_at_setup=seg.specialised, setup_s_including_specialisation=t_spec,
               trace_gen_ms_per_segment=last["gen_s"] / units * 1e3, prove_ms_per_segment=last["prove_s"] / units * 1e3,
               input_staging_ms_per_segment=last["stage_s"] / units * 1e3, distinct_segments=True,
               distinct_commitments_in_merge=len({tuple(int(x) for x in r) for r in last["merged"]}),
               cells_per_s_prove_only=cells_mine * steps / last["prove_s"] if last["prove_s"] else None,
               warmup=warmup, logup=bool(logup), proof_bytes_per_segment=int(last["words"]) * 4, per_rank_ms=per_rank_ms, ranks=world,
               widths=f"{min(s[1] for s in air_shapes)}..{max(s[1] for s in air_shapes)} (sum {sum(s[1] for s in air_shapes)})",
               log_heights=f"{min(min(h) for h in heights)}..{max(max(h) for h in heights)}",
               constraints=sum(s[3] for s in air_shapes), interactions=sum(s[4] for s in air_shapes), source_bytes=seg.source_bytes,
               prover_device_bytes=seg.device_bytes(), stage_ms_rank0=stage,
               stage_ms_note="per-kernel elapsed times; the per-AIR stages of a segment run on side streams (POWDR_SEGMENT_STREAMS, default 4) and "
                             "overlap, so the sum exceeds the wall time of the step",
               note="per unit: the segment's own inputs staged on the device (seeded by the segment's index: same AIRs, other rows — the segments of one "
                    "execution), trace generation of every AIR + one pw-stark v1 proof, all timed; one segment's buffers resident per rank; "
                    "value = all segments of all ranks / max-over-ranks time. AIRs: synthetic APCs with "
                    "generated traces, the 13 RV32IM instruction AIRs with the reference's real constraints / interactions on traces expanded from "
                    "records, the 3 lookup periphery AIRs from the histograms; the other 5 system AIRs of the reference's 19 (connector, program, "
                    "memory boundary, Merkle, Poseidon2: 357 of 819 columns) are external chips and are left out")
    LAST_OUTPUTS["segment_commitments"] = np.array(last["merged"], copy=True)
    prover.set_device_budget(0)
    if rank == 0 and checks:
        _segment_checks(seg, list(last["mine"]), rec, shapes=shapes)
    seg.close()
    import gc

    del seg
    gc.collect()
    torch.cuda.empty_cache()
    return rec if rank == 0 else None


def c3_leg(queries, pow_bits, steps=2, constraints_only_too=True, segment_too=True):
    """BASELINE configs[2] (guest-ecrecover autoprecompile, 2^22 rows — the reference's default segment height,
    openvm-riscv/src/lib.rs:366-371 — "HBM-roofline report") inside the driver-timed line, WITH its bus interactions inside the proof
    (PowdrAir::eval always pushes them, chip.rs:117-129): the C3 AIR (3 731 columns, 3 114 constraints, 2 314 bus interactions = 1 157
    LogUp groups = 4 632 permutation columns; W * H > 2^32, column-index operands) on dense synthetic sources (`C3p`: the real block's
    ~600 GB of dummy traces fit no single GPU — SURVEY.md §8 row f-1). The resident LDE of 8 363 committed columns x 2^23 rows would be
    280 GB, so the prover runs STREAMED (include/powdr_prover.h): coefficient arrays resident, the extended domain walked as 2^b
    sub-cosets. One trace generation + 1 warm-up proof + `steps` timed proofs, host-verified; per-kernel table; and (sub-record
    `constraints_only`) the round-3 figure: the resident constraints-only proof of the same trace."""
    from powdr_amd import abi, prover

    free = torch.cuda.mem_get_info()[0]
    if free < 250e9:
        return dict(skipped=f"needs ~250 GB of HBM for 3 731 x 2^22 with the bus argument (trace 62.6 GB + streamed prover ~185 GB); {free / 1e9:.0f} GB free")
    log_h = 22
    wl = build_workload("C3p", log_h, False, seed=0)
    W, H = wl["W"], wl["H"]
    torch.cuda.synchronize()
    abi.lib.powdr_gpu_timing_enable(1)
    t1 = time.perf_counter()
    wl["apc"].generate_witness_gpu(wl["instr_air"], wl["dummy"], wl["calls"], wl["out"].data_ptr(), wl["per"])
    torch.cuda.synchronize()
    t_gen = time.perf_counter() - t1
    tg_timing = abi.timing_report()
    abi.lib.powdr_gpu_timing_enable(0)
    src_bytes = wl["src_bytes"]
    wl["dummy"].clear(); wl["tensors"].clear()  # the sources make room for the prover
    torch.cuda.empty_cache()
    cells = W * H
    algo = {"apc_gather_tile_kernel": 8.0, "ntt_group_kernel<dif>": 8.0, "lde_fused_kernel": 12.0, "ntt_group_kernel<dit>": 16.0, "leaf_hash_kernel": 8.0,
            "deep_kernel": 8.0, "ext_dot_partial_kernel": 4.0, "ext_lincomb_kernel": 4.0}

    def kernel_table(timing, n, committed_cells):
        out = {}
        for k, (cnt, ms) in sorted(timing.items(), key=lambda kv: -kv[1][1]):
            e = dict(launches_per_step=cnt / n, ms=ms / n)
            if k in algo:
                e["algorithmic_GBps"] = algo[k] * committed_cells / (ms / n * 1e-3) / 1e9
                e["frac_of_hbm_peak"] = e["algorithmic_GBps"] / HBM_PEAK_GBS
            out[k] = e
        return out

    def run(pr, n, verify, consume=False):
        """1 warm-up + n timed proofs. consume: pw_prover_prove_consuming — the trace is handed over, as the reference hands `common_main`
        to its engine (cuda/mod.rs:415-419); a streamed proof leaves the trace's coefficient arrays in its place, and the trace is
        restored from them (pw_trace_from_coefficients, exact) OUTSIDE the timed region before the next proof."""
        ptr = wl["out"].data_ptr()
        eaten = consume and pr.stream_log_blocks_consuming(log_h) > 0

        def restore():
            if eaten:
                prover.trace_from_coefficients(ptr, W, log_h)

        pr.prove(ptr, log_h, copy=False, consume=consume)  # warm-up: allocation of the prover's buffers
        torch.cuda.synchronize()
        restore()
        timing, t_total, proof = {}, 0.0, None
        for _ in range(n):
            torch.cuda.synchronize()
            abi.lib.powdr_gpu_timing_enable(1)
            t2 = time.perf_counter()
            proof = pr.prove(ptr, log_h, consume=consume)
            torch.cuda.synchronize()
            t_total += time.perf_counter() - t2
            for k, (cnt, ms) in abi.timing_report().items():
                c0, m0 = timing.get(k, (0, 0.0))
                timing[k] = (c0 + cnt, m0 + ms)
            abi.lib.powdr_gpu_timing_enable(0)
            restore()
        return t_total / n, timing, proof, verify(proof)

    # ---- the proof with the bus argument (streamed) ----
    it = wl["apc"].compile_bus(1)
    perm_cols = 4 * len(prover.logup_group_starts(it))
    pr = prover.Prover(W, *wl["cons"], num_queries=queries, pow_bits=pow_bits, interactions=it)
    t0 = time.perf_counter()
    pr.specialise()
    t_spec = time.perf_counter() - t0
    consume = not os.environ.get("POWDR_BENCH_C3_KEEP_TRACE")
    checksum0 = int(wl["out"].view(torch.int64).sum().item())
    t_prove, timing, proof, rc = run(pr, steps, lambda pf: prover.verify_logup(pf, W, log_h, *wl["cons"], it, num_queries=queries, pow_bits=pow_bits)[0],
                                     consume=consume)
    mode = pr.stream_log_blocks_consuming(log_h) if consume else pr.stream_log_blocks(log_h)
    trace_restored = int(wl["out"].view(torch.int64).sum().item()) == checksum0
    step_s = t_prove + t_gen
    rho = perm_cols / W
    bpc = 48.0 + 4.0 + 44.0 * rho
    rec = dict(workload=f"C3p guest-ecrecover-shaped AIR: {W} cols x 2^{log_h} rows, {len(wl['cons'][1])} constraints, {wl['apc'].n_bus} bus interactions "
                        f"INSIDE the proof ({perm_cols} permutation columns), dense synthetic sources ({src_bytes / 1e9:.1f} GB, released after trace generation)",
               logup=True, cells=cells, steps=steps, warmup=1, trace_gen_ms=t_gen * 1e3, prove_ms=t_prove * 1e3, value=cells / step_s, unit="cells/s",
               cells_per_s_prove_only=cells / t_prove, verify_rc=int(rc), specialised_kernels=pr.specialised(), specialise_s=t_spec,
               stream_log_blocks=mode, trace_handed_over=bool(consume), trace_restored_between_proofs=bool(trace_restored),
               mode=(f"streamed: coefficient arrays resident, extended domain walked as {1 << mode} sub-cosets per pass (commit main, commit perm, quotient, queries)"
                     if mode > 0 else "resident LDE"),
               committed_columns=W + perm_cols + 8, trace_bytes=cells * 4, prover_device_bytes=pr.device_bytes(),
               prover_plus_trace_bytes=pr.device_bytes() + cells * 4,
               whole_step_hbm=dict(algo_bytes_per_main_cell=bpc, rho=rho, achieved_GBps=cells / step_s * bpc / 1e9, peak_GBps=HBM_PEAK_GBS,
                                   frac=cells / step_s * bpc / 1e9 / HBM_PEAK_GBS,
                                   note="SURVEY 8d: 48 + 4 + 44 rho bytes per main cell; the streamed mode re-extends every column for each of its passes, "
                                        "so the bytes it moves are higher than the resident figure this fraction is priced against"),
               proof_bytes=int(len(proof) * 4), kernels=kernel_table(timing, steps, (W + perm_cols + 8) * H))
    for k, (cnt, ms) in tg_timing.items():
        e = dict(launches_per_step=cnt, ms=ms)
        if k in algo:
            e["algorithmic_GBps"] = algo[k] * cells / (ms * 1e-3) / 1e9
            e["frac_of_hbm_peak"] = e["algorithmic_GBps"] / HBM_PEAK_GBS
        rec["kernels"][k] = e
    pr.close()
    torch.cuda.empty_cache()
    # ---- the same AIR inside ONE SEGMENT PROOF with the periphery AIRs its lookups go to (pw_prove_segment, pw-stark v1): the shape of
    # the reference's per-segment engine call. The APC AIR is the only one of its height and is streamed inside the segment proof.
    if segment_too:
        try:
            from powdr_amd import periphery as per_

            p_ = wl["per"]
            empty = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))
            traces = [wl["out"], per_.var_range_trace(p_.var_hist), per_.tuple2_trace(p_.tuple_hist, p_.tuple_sizes), per_.bitwise_trace(p_.bitwise_hist)]
            descs = [(W, log_h, wl["cons"][0], wl["cons"][1], it),
                     (3, p_.var_hist.numel().bit_length() - 1, *empty, per_.var_range_interactions(p_.var_bus)),
                     (3, p_.tuple_hist.numel().bit_length() - 1, *empty, per_.tuple2_interactions(p_.tuple_bus)),
                     (5, 16, *empty, per_.bitwise_interactions(p_.bitwise_bus))]
            provers = [prover.Prover(w, bc, sp, num_queries=queries, pow_bits=pow_bits, interactions=ia) for (w, lh, bc, sp, ia) in descs]
            seg = [(pr_, t.data_ptr(), d[1]) for pr_, t, d in zip(provers, traces, descs)]
            # pw_prove_segment_consuming (round 6): the APC chip moves its trace into the engine like the reference's (cuda/mod.rs:415-419) — the
            # streamed AIR keeps its coefficient arrays in the trace's own buffer (two sub-cosets instead of four); restored outside the timed region
            hand = [True, False, False, False]

            def restore():
                modes = prover.segment_last_modes()
                if modes and modes[0][1]:
                    prover.trace_from_coefficients(wl["out"].data_ptr(), W, log_h)
                return modes

            prover.prove_segment(seg, logup=True, copy=False, hand_over=hand)  # warm-up: buffers, kernels
            torch.cuda.synchronize()
            restore()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            pf = prover.prove_segment(seg, logup=True, copy=True, hand_over=hand)
            t_seg = time.perf_counter() - t3
            modes = restore()
            plan = prover.segment_last_plan()
            seg_cells = sum(d[0] << d[1] for d in descs)
            rec["segment"] = dict(airs=len(descs), cells=seg_cells, prove_ms=t_seg * 1e3, cells_per_s_prove_only=seg_cells / t_seg,
                                  verify_rc=int(prover.verify_segment(descs, pf, queries, pow_bits, True)[0]), proof_bytes=int(len(pf) * 4),
                                  apc_air_stream_log_blocks=int(modes[0][0]), trace_handed_over=bool(modes[0][1]),
                                  plan_bytes=dict(all_resident=plan[0], as_planned=plan[1], available=plan[2]),
                                  prover_device_bytes=sum(x.device_bytes() for x in provers),
                                  note="ONE pw-stark v1 proof (pw_prove_segment_consuming) for {the C3 APC AIR with all its interactions, var-range, tuple and "
                                       "bitwise periphery AIRs from the histograms trace generation filled}; the APC AIR is streamed inside the segment proof "
                                       "with its trace handed over: its coefficient arrays stay in the caller's buffer")
            for x in provers:
                x.close()
            del traces, seg
            torch.cuda.empty_cache()
        except Exception as e:  # an extra
            rec["segment"] = dict(verify_rc=None, error=f"{type(e).__name__}: {e}")
            torch.cuda.empty_cache()
    # ---- the round-3 figure: constraints-only proof of the same trace, resident LDE ----
    if constraints_only_too:
        try:
            pr = prover.Prover(W, *wl["cons"], num_queries=queries, pow_bits=pow_bits)
            mode0 = pr.stream_log_blocks(log_h)
            t_p, timing0, proof0, rc0 = run(pr, 1, lambda pf: prover.verify(pf, W, log_h, *wl["cons"], num_queries=queries, pow_bits=pow_bits))
            rec["constraints_only"] = dict(logup=False, prove_ms=t_p * 1e3, value=cells / (t_p + t_gen), cells_per_s_prove_only=cells / t_p, verify_rc=int(rc0),
                                           stream_log_blocks=mode0, prover_device_bytes=pr.device_bytes(), proof_bytes=int(len(proof0) * 4),
                                           kernels=kernel_table(timing0, 1, (W + 8) * H),
                                           note="a weaker statement than `value`: the bus interactions are replayed into the histograms but not proven")
            pr.close()
        except Exception as e:  # an extra
            rec["constraints_only"] = dict(value=None, error=f"{type(e).__name__}: {e}")
    wl.clear()
    torch.cuda.empty_cache()
    return rec


LAST_OUTPUTS = {}  # name -> array: what the last timed step of the headline computed (--dump-outputs)
DUMP_LIMIT = 64 << 20  # bytes over all files


def dump_outputs(out_dir, rank):
    """--dump-outputs DIR: LAST_OUTPUTS as DIR/<name>.npy in float64 (exact for u32 words), rank 0 only."""
    if not out_dir or rank != 0:
        return
    d = Path(out_dir)
    d.mkdir(parents=True, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in LAST_OUTPUTS.items()}
    total = sum(a.nbytes for a in arrays.values())
    assert arrays and total <= DUMP_LIMIT, f"--dump-outputs: {total} bytes in {sorted(arrays)}"
    for k, a in arrays.items():
        np.save(d / f"{k}.npy", a)


def build_info():
    """How the library this process loaded was built (the driver's build() runs before the bench; *.so is git-ignored and travels
    with the snapshot): path, size, age relative to its sources, and whether hipcc is present to rebuild it here."""
    import hashlib
    import shutil

    from powdr_amd import build as b

    lib = b.LIB
    srcs = list(b.CSRC.glob("*.hip")) + list(b.CSRC.glob("*.hpp")) + list((b.CSRC / "host").glob("*.cpp"))
    newest = max((f.stat().st_mtime for f in srcs), default=0.0)
    return dict(lib=str(lib.relative_to(ROOT)), bytes=lib.stat().st_size, sha256_16=hashlib.sha256(lib.read_bytes()).hexdigest()[:16],
                built_after_newest_source=bool(lib.stat().st_mtime >= newest), hipcc_present=bool(shutil.which("hipcc") or Path(b.HIPCC).exists()),
                build_mode="in-tree, hipcc --offload-arch=gfx950 (powdr_amd/build.py via __graft_entry__.build()); the bench loads this prebuilt .so, "
                           "expression kernels are additionally specialised at run time with hiprtc")


def live_pmc_leaf_hash(width: int, log_n: int):
    """The dominant kernel's PMC counters measured IN THIS RUN: two short rocprofv3 --pmc passes (FETCH_SIZE; SQ_INSTS_VALU — one
    counter set per pass, MI355X_MICROARCH.md) of tools/leaf_hash_once.py, which launches leaf_hash_kernel on a matrix of the
    timed shape. Returns {"fetch_bytes_per_launch", "valu_instr_per_launch", "launches"} or None (no rocprofv3, a failing pass)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    exe = shutil.which("rocprofv3")
    script = Path(__file__).resolve().parent / "tools" / "leaf_hash_once.py"
    if not exe or not script.exists():
        return None
    out = {}
    env = dict(os.environ, TMPDIR="/tmp")
    for counter in ("FETCH_SIZE", "SQ_INSTS_VALU"):
        tmp = tempfile.mkdtemp(prefix="powdr_pmc_", dir="/tmp")
        try:
            subprocess.run([exe, "--pmc", counter, "--output-format", "csv", "-d", tmp, "--", sys.executable, str(script), str(width), str(log_n)],
                           cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300, check=True)
            total, disp = 0.0, set()
            for f in glob.glob(tmp + "/**/*counter_collection.csv", recursive=True):
                for r in csv.DictReader(open(f)):
                    if r["Counter_Name"] == counter and "leaf_hash_kernel" in r["Kernel_Name"]:
                        total += float(r["Counter_Value"])
                        disp.add(r["Dispatch_Id"])
            if not disp:
                return None
            out[counter] = total / len(disp)
            out["launches"] = len(disp)
        except Exception:
            return None
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    # FETCH_SIZE: KiB, and on gfx950 wide coalesced streaming reads are tallied at half their bytes (same guide, HBM section)
    return dict(fetch_bytes_per_launch=out["FETCH_SIZE"] * 1024 * 2, valu_instr_per_launch=out["SQ_INSTS_VALU"], launches=out["launches"])


def load_profile_json(name):
    f = ROOT / "profiles" / name
    try:
        return json.loads(f.read_text()) if f.exists() else None
    except Exception:
        return None


def main():
    global SEGMENT_SHAPES, SEGMENT_BUDGET_FRAC, SPECIALISE_ALL
    args = parse_args()
    SEGMENT_SHAPES, SEGMENT_BUDGET_FRAC = args.segment_shapes, args.segment_budget_frac
    SPECIALISE_ALL = bool(args.segment_jit_all)
    self_launch(args)  # --gpus N > 1 without a launcher: re-run as N ranks (does not return)
    if args.launch_check:
        launch_check()
        return
    if int(os.environ.get("WORLD_SIZE", "1")) != max(1, args.gpus) and not args.inproc:
        print(f"bench.py: --gpus {args.gpus} but the launcher started {os.environ.get('WORLD_SIZE', '1')} rank(s)", file=sys.stderr)
        sys.exit(2)
    phase("main: arguments parsed")
    rank, local, world = setup_distributed(args.gpus)
    phase("process group up")
    from powdr_amd import abi, prover, synth
    phase("library loaded")

    def barrier():
        if world > 1:
            import torch.distributed as dist

            dist.barrier()
        torch.cuda.synchronize()

    if args.shape in ("C4", "C5") and args.inproc and world == 1:
        rec = segment_bench_inproc(args.shape, args.segments, args.segment_log_height, args.steps, args.warmup, args.logup, args.queries,
                                   args.pow_bits, max(1, args.gpus), abi, checks=args.full)
        dump_outputs(args.dump_outputs, 0)
        whole = rec["value"] / max(1, args.gpus) * ALGO_BYTES_PER_CELL / 1e9
        emit(dict(
            metric="STARK cells/sec (trace rows x cols), multi-segment " + ("guest-pairing-shaped" if args.shape == "C4" else "reth-shaped")
                   + (" [with the bus argument]" if args.logup else " [constraints-only proofs]"),
            value=rec["value"], unit="cells/s", n_gpus=max(1, args.gpus), steps=args.steps, warmup=args.warmup, ms_per_step=rec["ms_per_step"],
            higher_is_better=True, scaling="strong", vs_baseline=None, dtype="u32 (BabyBear, Montgomery)", data="synthetic",
            metric_short=f"STARK cells/sec (trace rows x cols), multi-segment {args.shape}" + (" [with the bus argument]" if args.logup else " [constraints-only]"),
            config=dict(workload_short=f"{args.shape}: {args.segments} segments x {rec['airs_per_segment']} AIRs, one proof per segment, {rec['workers']} in-process workers",
                        workload=f"{args.shape}: {args.segments} segments x {rec['airs_per_segment']} AIRs (up to {rec['cells_per_segment']} cells, {rec['cells_per_step']} in all), one proof "
                                 f"per segment, {rec['workers']} in-process workers on devices {rec['devices']} (pw_prove_segments_multi)",
                        parallelism=f"segments over {rec['workers']} host threads in one process (strong)", proof_bytes=rec["proof_bytes_per_segment"]),
            roofline=dict(bound="hbm", kernel="whole step", achieved=whole, peak=HBM_PEAK_GBS, unit="GB/s", frac=whole / HBM_PEAK_GBS, traffic=None,
                          algo_bytes_per_cell=ALGO_BYTES_PER_CELL, note="per GPU, 48 B per cell"),
            cpu_baseline=None, multi_segment=rec))
        return
    if args.shape in ("C4", "C5"):
        # BASELINE configs[3] / configs[4]: multi-AIR segments sharded over the GPUs of the node, strong scaling
        rec = segment_bench(args.shape, args.segments, args.segment_log_height, args.steps, args.warmup, args.logup, args.queries,
                            args.pow_bits, rank, world, abi, barrier, checks=args.full)
        dump_outputs(args.dump_outputs, rank)
        jit_cache = jit_cache_by_rank(world)
        if rank == 0:
            whole = rec["value"] / world * ALGO_BYTES_PER_CELL / 1e9
            line = dict(metric="STARK cells/sec (trace rows x cols), multi-segment " + ("guest-pairing-shaped" if args.shape == "C4" else "reth-shaped")
                               + (" [with the bus argument]" if args.logup else " [constraints-only proofs]"),
                        value=rec["value"], unit="cells/s", n_gpus=world, steps=args.steps, warmup=args.warmup, ms_per_step=rec["ms_per_step"],
                        higher_is_better=True, scaling="strong", vs_baseline=None, dtype="u32 (BabyBear, Montgomery)", data="synthetic",
                        rccl_ranks=comm_facts(world)["ranks"], comm=comm_facts(world), per_rank_ms=rec.get("per_rank_ms"),
                        metric_short=f"STARK cells/sec (trace rows x cols), multi-segment {args.shape}" + (" [with the bus argument]" if args.logup else " [constraints-only]"),
                        config=dict(workload_short=f"{args.shape}: {args.segments} segments x {rec['airs_per_segment']} AIRs, one proof per segment, sharded over {world} GPU(s) by cells",
                                    workload=f"{args.shape}: {args.segments} segments x {rec['airs_per_segment']} AIRs (up to {rec['cells_per_segment']} cells, {rec['cells_per_step']} in all, "
                                             f"heights 2^{rec['log_heights']}, widths {rec['widths']}), one proof per segment, segments sharded over "
                                             f"{world} GPU(s) by cells, main commitments all-gathered",
                                    parallelism=f"segments over {world} ranks (strong)", proof_bytes=rec["proof_bytes_per_segment"]),
                        roofline=dict(bound="hbm", kernel="whole step", achieved=whole, peak=HBM_PEAK_GBS, unit="GB/s", frac=whole / HBM_PEAK_GBS,
                                      traffic=None, algo_bytes_per_cell=ALGO_BYTES_PER_CELL, note="per GPU, 48 B per cell (proof stages only use 40 of them)"),
                        cpu_baseline=None, multi_segment=rec, jit_cache=jit_cache)
            emit(line)
        if world > 1:
            import torch.distributed as dist

            dist.destroy_process_group()
        return

    shape = synth.SHAPES[args.shape]
    log_h = args.log_height or shape.log_height
    try:
        # every rank proves the SAME AIR (the execution's APC: seed 0) on its OWN segment's values (data_seed = rank) — one set of
        # specialised kernels for the node, compiled by rank 0 and loaded by the others
        wl = build_workload(args.shape, log_h, args.exact_source_heights, seed=0, calls_fraction=args.calls_fraction, data_seed=rank)
    except torch.cuda.OutOfMemoryError:
        # power-of-two source heights (like the original chips' traces) need 150 GB at C2; fall back to
        # b*calls-row sources (115 GB) rather than fail — same kernels, same cells, noted in config.workload
        torch.cuda.empty_cache()
        args.exact_source_heights = True
        wl = build_workload(args.shape, log_h, True, seed=0, calls_fraction=args.calls_fraction, data_seed=rank)
    phase("workload built")
    all_inter = wl["apc"].compile_bus(1)  # (interactions, spans, bytecode) with column operands
    lg_perm_cols = 4 * len(prover.logup_group_starts(all_inter))  # 4 * (groups + 1)
    inter = all_inter if args.logup else None
    perm_cols = lg_perm_cols if args.logup else 0
    pr = prover.Prover(wl["W"], *wl["cons"], num_queries=args.queries, pow_bits=args.pow_bits, interactions=inter)
    from powdr_amd import sharding

    # run-time specialisation (hiprtc) is plan work like the tables: done before any step, timed or not. On a multi-rank node rank 0
    # compiles first, so that the other ranks find the code objects in the shared on-disk compiler cache instead of compiling the same
    # sources N times next to each other
    if rank == 0 and log_h >= 18:
        pr.specialise()
    barrier()
    if rank != 0 and log_h >= 18:
        pr.specialise()

    def run_segment(w, with_logup):
        w["per"].zero()
        w["apc"].generate_witness_gpu(wl["instr_air"], wl["dummy"], wl["calls"], w["out"].data_ptr(), w["per"])
        proof = w["pr"].prove(w["out"].data_ptr(), log_h, copy=False)
        if world > 1:
            # the final commitment merge: all-gather of the per-segment trace roots (32 B per segment)
            o = 7 if with_logup else 6
            sharding.merge_commitments([rank], proof[o:o + 8].reshape(1, 8), world)
        return proof

    main_worker = dict(apc=wl["apc"], per=wl["per"], out=wl["out"], pr=pr)
    workers = [main_worker]
    if args.pipeline > 1:
        import threading

        from powdr_amd import host, tracegen as tg

        main_worker["stream"] = torch.cuda.Stream()
        for _ in range(args.pipeline - 1):
            workers.append(dict(stream=torch.cuda.Stream(), apc=host.Apc(wl["synth"].doc), per=tg.Periphery.fresh(),
                                out=torch.empty_like(wl["out"]),
                                pr=prover.Prover(wl["W"], *wl["cons"], num_queries=args.queries, pow_bits=args.pow_bits,
                                                 interactions=inter)))

    last = {}

    def run_steps(n):
        """n segments on this GPU: sequentially, or split over the pipeline's host threads/streams."""
        if args.pipeline == 1:
            for _ in range(n):
                last["proof"] = run_segment(main_worker, args.logup)
            return

        def body(w, k):
            with torch.cuda.stream(w["stream"]):
                abi.lib.powdr_gpu_set_stream(w["stream"].cuda_stream)
                for _ in range(k):
                    last["proof"] = run_segment(w, args.logup)

        counts = [n // len(workers) + (1 if i < n % len(workers) else 0) for i in range(len(workers))]
        th = [threading.Thread(target=body, args=(w, k)) for w, k in zip(workers, counts) if k]
        [t.start() for t in th]
        [t.join() for t in th]

    phase("headline: warm-up + timed steps start")
    elapsed, timing = timed_leg(run_steps, args.steps, max(args.warmup, len(workers) if args.warmup else 0), barrier, abi, world)
    phase("headline: done")
    if args.dump_outputs and rank == 0:
        # what a caller of the step receives from the last timed step: the proof words, the periphery histograms, and the trace (a fixed
        # seeded sample of its cells: the whole of it is 8 GB at C2). Taken now, before any other leg reuses the buffers.
        LAST_OUTPUTS["proof_words"] = np.array(last["proof"], copy=True)
        per = main_worker["per"]
        for name in ("var_hist", "tuple_hist", "bitwise_hist"):
            LAST_OUTPUTS["periphery_" + name] = getattr(per, name).cpu().numpy().view(np.uint32)
        flat = main_worker["out"].reshape(-1)
        pick = np.sort(np.random.default_rng(20261015).integers(0, flat.numel(), size=min(flat.numel(), 1 << 20), dtype=np.int64))
        LAST_OUTPUTS["trace_sample"] = flat[torch.from_numpy(pick).to(flat.device)].cpu().numpy().view(np.uint32)
    dump_outputs(args.dump_outputs, rank)
    per_rank_ms = [t / args.steps * 1e3 for t in LAST_PER_RANK_S]
    cells_per_step = wl["W"] * wl["H"]
    total_cells = cells_per_step * args.steps * world
    value = total_cells / elapsed
    proof_bytes = int(len(last["proof"]) * 4)
    prover_bytes = pr.device_bytes()

    # ---- trace generation from CALL-MAJOR COMPACTED sources (layout half; powdr_apc_tracegen_callmajor):
    # the same APC trace gathered from buffers that hold, per call, only the cells the APC uses. Not part of `value`: the
    # reference hands over full column-major dummy traces (cuda/mod.rs:228-253) and the timed step above consumes those.
    callmajor_leg = None
    if not args.no_callmajor_leg and args.pipeline == 1:
        try:
            from powdr_amd import tracegen as tg

            subs, air_ids, rbs = wl["apc"].build_substitutions(wl["instr_air"])
            calls = wl["calls"]
            slots = [dict() for _ in air_ids]
            subs_cm = np.zeros((len(subs), 3), np.int32)
            for i, (a, col, row, apc_col) in enumerate(subs):
                d = slots[a]
                subs_cm[i] = (a, d.setdefault((int(row), int(col)), len(d)), apc_col)
            cm_airs, cm_bytes = [], 0
            for k, d in enumerate(slots):
                ptr, w, h = wl["dummy"][int(air_ids[k])]
                t = next(tt for tt, ww, hh, bb in wl["tensors"].values() if tt.data_ptr() == ptr)
                U, b = len(d), int(rbs[k])
                base = torch.tensor([col * h + row for (row, col) in d], dtype=torch.int64, device="cuda")
                buf = torch.empty(calls * U, dtype=torch.int32, device="cuda")
                view = buf.view(calls, U)
                for r0 in range(0, calls, 1 << 15):  # chunks keep the index tensor small
                    r = torch.arange(r0, min(calls, r0 + (1 << 15)), device="cuda", dtype=torch.int64)
                    view[r0:r0 + len(r)] = t[base[None, :] + (r * b)[:, None]]
                cm_airs.append((buf, U))
                cm_bytes += buf.numel() * 4
            out2 = tg.DeviceMatrix(torch.empty_like(wl["out"]), wl["H"], wl["W"])
            tg.apc_tracegen_callmajor(out2, cm_airs, subs_cm, calls)  # warm-up + plan
            torch.cuda.synchronize()
            abi.lib.powdr_gpu_timing_enable(1)
            for _ in range(3):
                tg.apc_tracegen_callmajor(out2, cm_airs, subs_cm, calls)
            torch.cuda.synchronize()
            cm_ms = abi.timing_report()["apc_gather_callmajor_kernel"][1] / 3
            abi.lib.powdr_gpu_timing_enable(0)
            # same cells as the reference-layout gather wrote (derived columns aside: compare the substituted columns)
            cols = sorted(set(int(c) for c in subs_cm[:, 2]))
            same = all(torch.equal(out2.buf[c * wl["H"]:(c + 1) * wl["H"]], wl["out"][c * wl["H"]:(c + 1) * wl["H"]]) for c in cols[:: max(1, len(cols) // 64)])
            moved = cm_bytes + len(cols) * wl["H"] * 4
            callmajor_leg = dict(gather_ms=cm_ms, source_bytes=cm_bytes, cells_per_call=int(sum(len(d) for d in slots)),
                                 moved_GBps=moved / (cm_ms * 1e-3) / 1e9, frac_of_hbm_peak=moved / (cm_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                 equals_reference_layout_gather=bool(same),
                                 reference_layout_gather_ms=timing.get("apc_gather_tile_kernel", (0, 0.0))[1] / args.steps,
                                 reference_layout_source_bytes=wl["src_bytes"],
                                 note="powdr_apc_tracegen_callmajor: sources = per call only the cells the APC uses, contiguous; what the original "
                                      "chips would have to write for the gather to move 8 B per APC cell (SURVEY 8d) instead of the whole dummy traces")
            del out2, cm_airs, buf, view, t, base
            torch.cuda.empty_cache()
        except Exception as e:
            callmajor_leg = dict(gather_ms=None, error=f"{type(e).__name__}: {e}")

    # ---- the reference-layout gather on COLUMN-STRUCTURED substitutions: same dummy traces, same _apc_tracegen, but the
    # surviving cells are few columns of each original AIR present in most instructions — the structure of the reference's own
    # optimised-APC snapshots (synth.column_structured_substitutions cites them) — instead of cells scattered uniformly over the
    # block (the timed step's workload: every sector of every source column is touched). Not part of `value`.
    colstruct_leg = None
    if not args.no_callmajor_leg and args.pipeline == 1:
        try:
            from powdr_amd import synth as _synth, tracegen as tg

            subs0, air_ids, rbs = wl["apc"].build_substitutions(wl["instr_air"])
            calls = wl["calls"]
            dims, airs_cs = [], []
            for k in range(len(air_ids)):
                ptr, w, h = wl["dummy"][int(air_ids[k])]
                t = next(tt for tt, ww, hh, bb in wl["tensors"].values() if tt.data_ptr() == ptr)
                dims.append((w, int(rbs[k])))
                airs_cs.append((t, w, h, int(rbs[k])))
            subs_cs = _synth.column_structured_substitutions(dims, len(subs0), seed=1)
            out2 = tg.DeviceMatrix(torch.zeros_like(wl["out"]), wl["H"], wl["W"])
            keep = tg.apc_tracegen(out2, airs_cs, subs_cs, calls)  # warm-up + plan
            torch.cuda.synchronize()
            abi.lib.powdr_gpu_timing_enable(1)
            for _ in range(3):
                keep = tg.apc_tracegen(out2, airs_cs, subs_cs, calls)
            torch.cuda.synchronize()
            cs_ms = abi.timing_report()["apc_gather_tile_kernel"][1] / 3
            abi.lib.powdr_gpu_timing_enable(0)
            ok = True
            r = torch.arange(0, calls, device="cuda", dtype=torch.int64)
            for a, col, row, apc_col in subs_cs[:: max(1, len(subs_cs) // 48)].tolist():
                t, w, h, b = airs_cs[a]
                ok = ok and torch.equal(out2.buf[apc_col * wl["H"]: apc_col * wl["H"] + calls], t[col * h + row + r * b])
            used_cols = len(set((int(a), int(c)) for a, c, _, _ in subs_cs))
            src_touched = sum(airs_cs[a][2] * 4 for a, c in set((int(a), int(c)) for a, c, _, _ in subs_cs))
            colstruct_leg = dict(gather_ms=cs_ms, substitutions=int(len(subs_cs)), source_columns_used=used_cols,
                                 source_columns_total=int(sum(w for w, _ in dims)), source_bytes_touched=int(src_touched),
                                 matches_direct_indexing=bool(ok),
                                 scattered_gather_ms=timing.get("apc_gather_tile_kernel", (0, 0.0))[1] / args.steps,
                                 step_ms_with_this_gather=elapsed / args.steps * 1e3 - timing.get("apc_gather_tile_kernel", (0, 0.0))[1] / args.steps + cs_ms,
                                 note="_apc_tracegen on the reference's source layout with column-structured substitutions (few columns of every "
                                      "original AIR, present in ~65 % of its instructions: what optimised APCs look like in the reference's snapshots); "
                                      "the timed step uses uniformly scattered cells, the worst case for the gather")
            del out2, keep, airs_cs, t
            torch.cuda.empty_cache()
        except Exception as e:
            colstruct_leg = dict(gather_ms=None, error=f"{type(e).__name__}: {e}")

    # ---- second timed leg: the same step with the OTHER proof kind. Headline (default): the proof includes the bus interactions
    # PowdrAir::eval pushes (chip.rs:117-129) — the statement the reference's backend proves; second leg: the constraints-only proof
    # (north_star's kernel list: NTT, quotient, Merkle, FRI — no permutation phase). Same inputs, same trace generation.
    other_leg = None
    other_logup = not args.logup
    if not args.no_logup_leg and args.pipeline == 1:
        pr.close()
        torch.cuda.empty_cache()
        try:
            pr_o = prover.Prover(wl["W"], *wl["cons"], num_queries=args.queries, pow_bits=args.pow_bits, interactions=all_inter if other_logup else None)
            o_worker = dict(apc=wl["apc"], per=wl["per"], out=wl["out"], pr=pr_o)
            o_last = {}

            def run_o(n):
                for _ in range(n):
                    o_last["proof"] = run_segment(o_worker, other_logup)

            o_elapsed, o_timing = timed_leg(run_o, args.logup_steps, 1, barrier, abi, world)
            rho = lg_perm_cols / wl["W"] if other_logup else 0.0
            o_bytes_per_cell = 48 + 4 + 44 * rho if other_logup else ALGO_BYTES_PER_CELL
            o_value = cells_per_step * args.logup_steps * world / o_elapsed
            o_stage = {k: ms / args.logup_steps for k, (c, ms) in o_timing.items()}
            other_leg = dict(
                value=o_value, unit="main cells/s", ms_per_step=o_elapsed / args.logup_steps * 1e3, steps=args.logup_steps, warmup=1,
                interaction_groups=(lg_perm_cols // 4 - 1) if other_logup else 0, perm_cols=lg_perm_cols if other_logup else 0, rho=rho,
                algo_bytes_per_main_cell=o_bytes_per_cell,
                whole_step_hbm=dict(achieved_GBps=o_value * o_bytes_per_cell / 1e9, peak_GBps=HBM_PEAK_GBS,
                                    frac=o_value * o_bytes_per_cell / 1e9 / HBM_PEAK_GBS),
                proof_bytes=int(len(o_last["proof"]) * 4), prover_device_bytes=pr_o.device_bytes(), stage_ms=o_stage,
                gauges=gauges_of(o_stage), specialised_kernels=pr_o.specialised(),
                note=("same segment, same trace generation, proof = pw-stark v0 + LogUp (proof magic PWS2): the AIR's bus interactions are "
                      "inside the proof (permutation columns, running sum, extended quotient, openings at zeta and g*zeta)") if other_logup else
                     ("same segment, same trace generation, CONSTRAINTS-ONLY proof (proof magic PWS1): the bus interactions are replayed into the "
                      "periphery histograms but are not inside the proof — the round-1/2 headline"))
            pr_o.close()
            o_worker.clear()
        except Exception as e:  # the extra leg must never take the headline down
            other_leg = dict(value=None, error=f"{type(e).__name__}: {e}")
    logup_leg = other_leg if other_logup else None
    constraints_only_leg = None if other_logup else other_leg

    # ---- trace generation FROM RECORDS (producer half): the original chips expand their records inside the
    # gather (powdr_apc_tracegen_records) — no dummy traces. Checked at full size against the reference flow on the same records:
    # powdr_original_airs_expand into the (now overwritten) source buffers, then the timed step's own gather. Not part of `value`.
    phase("second leg + call-major done")
    records_leg = None
    if not args.no_callmajor_leg and args.pipeline == 1 and args.shape == "C2":
        try:
            from powdr_amd import original_chips as oc_, tracegen as tg

            doc = wl["synth"].doc
            ins = oc_.sanitise_instructions(doc["block"]["blocks"][0]["instructions"])
            table = oc_.InstructionTable(ins, [len(x) > 0 for x in doc["subs"]], int(doc["block"]["blocks"][0]["start_pc"]))
            subs0, air_ids, rbs = wl["apc"].build_substitutions(wl["instr_air"])
            kinds = [oc_.KIND_NAMES.index(wl["air_names"][int(a)]) for a in air_ids]
            assert [table.row_block_size[k] for k in kinds] == [int(b) for b in rbs]
            rsubs, n_rs = table.record_substitutions(subs0, kinds)
            calls = wl["calls"]
            rec = oc_.random_records_device(table, calls, seed=3)
            out2 = torch.empty_like(wl["out"])
            oc_.tracegen_records(out2.data_ptr(), wl["H"], rec.data_ptr(), calls, table, rsubs, n_rs)  # warm-up + tables
            torch.cuda.synchronize()
            abi.lib.powdr_gpu_timing_enable(1)
            for _ in range(3):
                oc_.tracegen_records(out2.data_ptr(), wl["H"], rec.data_ptr(), calls, table, rsubs, n_rs)
            torch.cuda.synchronize()
            fused_ms = abi.timing_report()["apc_tracegen_records_kernel"][1] / 3
            # the reference flow on the same records: full dummy traces (into the source buffers), then the gather of the timed step
            bufs = [None] * oc_.N_KINDS
            for k, a in zip(kinds, air_ids):
                ptr, w, h = wl["dummy"][int(a)]
                bufs[k] = (ptr, h)
            abi.lib.powdr_gpu_timing_enable(1)
            oc_.expand(rec.data_ptr(), calls, table, bufs)
            torch.cuda.synchronize()
            expand_ms = abi.timing_report()["original_airs_expand_kernel"][1]
            abi.lib.powdr_gpu_timing_enable(0)
            wl["apc"].generate_witness_gpu(wl["instr_air"], wl["dummy"], calls, wl["out"].data_ptr(), None)
            torch.cuda.synchronize()
            cols = sorted(set(int(c) for c in subs0[:, 3]))
            H_ = wl["H"]
            same = all(torch.equal(out2[c * H_:(c + 1) * H_], wl["out"][c * H_:(c + 1) * H_]) for c in cols)
            moved = rec.numel() * 4 + len(cols) * H_ * 4
            records_leg = dict(fused_ms=fused_ms, record_bytes=int(rec.numel() * 4), record_bytes_per_call=table.words_per_call * 4,
                               instructions_with_cells=len(table), substitutions=int(n_rs), moved_GBps=moved / (fused_ms * 1e-3) / 1e9,
                               frac_of_hbm_peak=moved / (fused_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                               equals_expand_then_gather_at_full_size=bool(same), columns_compared=len(cols),
                               reference_flow_expand_ms=expand_ms, reference_flow_gather_ms=timing.get("apc_gather_tile_kernel", (0, 0.0))[1] / args.steps,
                               reference_flow_dummy_trace_bytes=wl["src_bytes"],
                               step_ms_with_trace_from_records=elapsed / args.steps * 1e3 - timing.get("apc_gather_tile_kernel", (0, 0.0))[1] / args.steps + fused_ms,
                               step_note="derived: the headline step with its gather kernel replaced by the fused kernel's time (the headline itself "
                                         "keeps _apc_tracegen, the entry point cuda_abi.rs binds); the MEASURED step from records is `timed_step`",
                               note="powdr_apc_tracegen_records: the original chips (all thirteen RV32IM instruction AIRs; every constraint and lookup of the "
                                    "reference's openvm_constraints.txt holds on their rows; this block uses BaseAlu, Shift, LoadStore, BranchEqual, JalLui) expand "
                                    "their records inside the gather; only the cells the APC keeps are written, straight into their columns. The reference flow materialises the full dummy traces first (reference_flow_expand_ms on the same "
                                    "records, strided writes like a chip's) and gathers them (reference_flow_gather_ms)")
            # ---- the step FROM RECORDS, timed: powdr_apc_generate_witness_from_records (a1-a3 in one call: fused chip
            # expansion + gather, derived columns, bus replay) + the same proof as the headline, `--logup-steps` steps after one warm-up,
            # between barrier + synchronize like every timed leg. The 150 GB of dummy traces are released first: this flow has none.
            try:
                from powdr_amd import host as host_

                for k in ("tensors", "dummy"):
                    wl[k].clear()
                del bufs
                torch.cuda.empty_cache()
                doc_r = dict(doc)
                blk_r = dict(doc["block"]["blocks"][0])
                blk_r["instructions"] = ins
                doc_r["block"] = dict(doc["block"], blocks=[blk_r])
                # the synthetic APC draws its substitutions uniformly over the original rows' cells; from RECORDS the cells hold the chips'
                # real values, so every bounded APC column (bit, byte, k-bit range) is re-targeted to a cell of its own row whose real
                # values respect the bound (original_chips.typed_substitutions) — as in a real APC, whose lookups are in range by construction
                doc_r["subs"], untyped = oc_.typed_substitutions(ins, doc["subs"], wl["synth"].kinds, int(blk_r["start_pc"]))
                apc_r = host_.Apc(doc_r)
                cons_r = apc_r.compile_constraints()
                pr_r = prover.Prover(wl["W"], *cons_r, num_queries=args.queries, pow_bits=args.pow_bits, interactions=apc_r.compile_bus(1) if args.logup else None)
                if log_h >= 18:
                    pr_r.specialise()
                r_last = {}

                def run_r(n):
                    for _ in range(n):
                        wl["per"].zero()
                        apc_r.generate_witness_from_records(rec.data_ptr(), calls, out2.data_ptr(), wl["per"])
                        r_last["proof"] = pr_r.prove(out2.data_ptr(), log_h, copy=False)
                        if world > 1:
                            o = 7 if args.logup else 6
                            sharding.merge_commitments([rank], r_last["proof"][o:o + 8].reshape(1, 8), world)

                r_elapsed, r_timing = timed_leg(run_r, args.logup_steps, 1, barrier, abi, world)
                r_stage = {k: ms / args.logup_steps for k, (c, ms) in r_timing.items()}
                tg_names = ("apc_tracegen_records_kernel", "apc_apply_derived_expr_kernel", "apc_apply_bus_kernel", "bus_histogram_kernel")
                records_leg["timed_step"] = dict(
                    ms_per_step=r_elapsed / args.logup_steps * 1e3, value=cells_per_step * args.logup_steps * world / r_elapsed, unit="main cells/s",
                    steps=args.logup_steps, warmup=1, logup=bool(args.logup), trace_gen_ms=sum(r_stage.get(k, 0.0) for k in tg_names),
                    stage_ms=r_stage, proof_bytes=int(len(r_last["proof"]) * 4), record_bytes=int(rec.numel() * 4),
                    prover_mode=pr_r.stream_log_blocks(log_h), typed_substitutions=True, bounded_columns_left_untyped=int(untyped),
                    note="TIMED: powdr_apc_generate_witness_from_records (the original chips' expansion fused into the gather + derived columns + bus "
                         "replay) + pw_prover_prove, records resident in HBM, no dummy traces anywhere; same instructions, constraints and "
                         "interactions as the headline, every bounded APC column fed from a cell of its instruction's row whose real values respect "
                         "the bound (typed_substitutions), so that the lookups are in range as a real APC's are (with the headline's uniformly drawn "
                         "cells the chips' operand words land in byte columns, 50 lookups per row leave the binned path and the replay takes 28 ms "
                         "instead of 5: profiles/r04_bench_c2.json of the untyped run)")
                pr_r.close()
                apc_r.close()
            except Exception as e:
                records_leg["timed_step"] = dict(ms_per_step=None, error=f"{type(e).__name__}: {e}")
            del out2, rec
            torch.cuda.empty_cache()
        except Exception as e:
            records_leg = dict(fused_ms=None, error=f"{type(e).__name__}: {e}")

    # ---- third leg: multi-AIR segments, strong scaling (BASELINE configs[3]: sharded multi-segment guest-pairing). Every rank takes
    # part; the single-AIR workload's 180 GB are released first.
    segment_leg = None
    if not args.no_segment_leg and args.pipeline == 1:
        try:
            pr.close()
            for k in ("tensors", "dummy", "out"):
                wl.pop(k, None)
            main_worker.clear()
            import gc

            gc.collect()
            torch.cuda.empty_cache()
            seg_log = min(args.segment_log_height, log_h)
            phase("records leg done; multi_segment starts")
            segment_leg = segment_bench("C4", args.segments, seg_log, args.segment_steps, 1, args.logup, args.queries, args.pow_bits, rank, world,
                                        abi, barrier)
        except Exception as e:  # must never take the headline down
            segment_leg = dict(value=None, error=f"{type(e).__name__}: {e}")

    # ---- fourth leg: BASELINE configs[2] at full size on rank 0 (one GPU; everything else has been released by now)
    c3 = None
    if rank == 0 and not args.no_c3_leg and not args.no_segment_leg and args.pipeline == 1 and args.shape == "C2" and log_h == 20:
        try:
            import gc

            for k in ("tensors", "dummy", "out"):  # (the segment leg may have failed before it released the 150 GB of sources)
                wl.pop(k, None)
            main_worker.clear()
            gc.collect()
            torch.cuda.empty_cache()
            c3 = c3_leg(args.queries, args.pow_bits)
        except Exception as e:  # must never take the headline down
            c3 = dict(value=None, error=f"{type(e).__name__}: {e}")
            torch.cuda.empty_cache()

    phase("multi_segment done")
    jit_cache = jit_cache_by_rank(world)
    if rank == 0:
        per_kernel = {k: (c, ms) for k, (c, ms) in timing.items()}
        dom = max(per_kernel, key=lambda k: per_kernel[k][1]) if per_kernel else None
        # SURVEY.md 8d, algorithmic HBM bytes per main cell and kernel. The quotient kernel is NOT listed: it reads only the
        # columns the constraints reference (PMC: 2.9 GB per step at C2, not 8 B x cells), so a per-cell figure does not describe it.
        algo_bytes_per_cell = {"leaf_hash_kernel": 8.0, "apc_gather_tile_kernel": 8.0, "apc_apply_bus_kernel": 4.0,
                               "ntt_group_kernel<dif>": 8.0, "lde_fused_kernel": 12.0, "ntt_group_kernel<dit>": 16.0, "deep_kernel": 8.0}
        stage_ms = {k: ms / args.steps for k, (c, ms) in per_kernel.items()}
        gauges = gauges_of(stage_ms)
        # kernels that run once per COMMITTED column (LDE, leaf hash, DEEP): with the LogUp phase the permutation matrix is
        # committed like the trace, so their algorithmic bytes are per (main + permutation) cell
        committed_scale = (wl["W"] + perm_cols) / wl["W"]
        per_committed = {"leaf_hash_kernel", "ntt_group_kernel<dif>", "lde_fused_kernel", "ntt_group_kernel<dit>", "deep_kernel", "deep_logup_kernel"}
        algo_bytes_per_cell["deep_logup_kernel"] = 8.0
        copy_gbs = None
        shared_device = world > 1 and torch.cuda.device_count() < world  # the one-GPU test hook (POWDR_DIST_BACKEND=gloo): N ranks on GPU 0
        if not args.no_copy_ceiling and not shared_device:
            # device-to-device copy ceiling of THIS box: 4 GiB copies, outside every timed region. (Not when several ranks
            # share one device: 8 x 8 GiB beside a caller that holds most of the HBM oversubscribes it, the driver then evicts whole
            # processes in turn — a 9 s run took 162 s, tools/_hold.sh in round 6.)
            a_ = torch.empty(1 << 30, dtype=torch.int32, device="cuda")
            b_ = torch.empty_like(a_)
            b_.copy_(a_)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(4):
                b_.copy_(a_)
            e1.record()
            torch.cuda.synchronize()
            copy_gbs = 4 * 2 * a_.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9
            del a_, b_
        # PMC profiles of THIS round's code (separate rocprofv3 --pmc passes of this command, tools/pmc_traffic_json.py and
        # tools/pmc_valu_json.py): HBM traffic per kernel and step; VALU instructions per Poseidon2 permutation
        tprof_name = "r04_pmc_traffic_c2.json" if args.logup else "r02_pmc_traffic_c2.json"  # per-kernel PMC traffic of the committed profile of this proof kind
        tprof = load_profile_json(tprof_name) if (args.shape == "C2" and log_h == 20) else None
        traffic_db = {}
        if tprof:
            for k, v in tprof["kernels"].items():
                base = k.split("<")[0]
                if base == "ntt_group_kernel":  # the library times DIF (inverse) and DIT (forward) launches separately
                    base += "<dif>" if k.split("<")[1].startswith("true") else "<dit>"
                if base.startswith("apc_apply_bus"):  # interpreter and fixed-shape kernels share one timer
                    base = "apc_apply_bus_kernel"
                traffic_db[base] = traffic_db.get(base, 0.0) + v["fetch_bytes_corrected"] + v["write_bytes"]
        live = None
        if dom == "leaf_hash_kernel" and world == 1 and not args.no_live_pmc:
            live = live_pmc_leaf_hash(wl["W"], log_h + 1)
        roof = None
        if dom:
            cnt, ms = per_kernel[dom]
            abc = algo_bytes_per_cell.get(dom, 8.0)
            bytes_step = abc * cells_per_step * (committed_scale if dom in per_committed else 1.0)  # summed over one step's launches of that kernel
            achieved = bytes_step / (ms / args.steps * 1e-3) / 1e9
            roof = dict(bound="hbm", kernel=dom, achieved=achieved, peak=HBM_PEAK_GBS, unit="GB/s", frac=achieved / HBM_PEAK_GBS,
                        traffic=(live["fetch_bytes_per_launch"] * committed_scale + 2 * wl["H"] * (8 * 4 + (3 if args.logup else 2) * 32)) if live else traffic_db.get(dom),
                        traffic_unit=("bytes per step: FETCH_SIZE (KiB x 1024 x 2, the gfx950 correction for wide coalesced reads) of the trace-tree launch, measured "
                                      "IN THIS RUN by a rocprofv3 --pmc pass of tools/leaf_hash_once.py"
                                      + (f", x {committed_scale:.3f} for the permutation-tree launch of the same kernel ({perm_cols} more columns)" if args.logup else "")
                                      + ", + the algorithmic bytes of the 8-column quotient-tree launch and of the digests written" if live else
                                      f"bytes per step (PMC, profiles/{tprof_name})" if tprof else None),
                        algorithmic_bytes_per_step=bytes_step, avg_launch_ms=ms / cnt, launches_per_step=cnt / args.steps,
                        algo_bytes_per_cell=abc)
            # the whole step against SURVEY 8d's headline figure: 48 algorithmic bytes per main cell
            whole_bpc = 48 + 4 + 44 * perm_cols / wl["W"] if args.logup else ALGO_BYTES_PER_CELL  # 48 + 4 + 44 rho with the LogUp phase
            roof["whole_step"] = dict(algo_bytes_per_cell=whole_bpc, achieved_GBps=value / world * whole_bpc / 1e9,
                                      peak_GBps=HBM_PEAK_GBS, frac=value / world * whole_bpc / 1e9 / HBM_PEAK_GBS,
                                      note="per GPU; the step is bound by integer VALU issue (Poseidon2, NTT), not by HBM")
            if dom == "leaf_hash_kernel":
                # The dominant kernel is integer-VALU bound. Its instruction count per permutation and the issue cost of its
                # opcode mix are MEASURED (PMC SQ_INSTS_VALU of this round's kernel; tools/microbench_opcodes.hip) and read
                # from profiles/ — nothing is hard-coded here; absent profile => null.
                vm = load_profile_json("r02_valu_model.json")
                perms = 2 * wl["H"] * ((wl["W"] + 7) // 8) + 2 * wl["H"]  # trace LDE rows + 8-col quotient LDE rows
                perms += 2 * wl["H"] * ((perm_cols + 7) // 8)            # + the permutation matrix's rows (--logup)
                if vm and live:  # instructions per permutation as counted in this run (SQ_INSTS_VALU of the trace-tree launch)
                    vm = dict(vm, valu_instr_per_perm=live["valu_instr_per_launch"] / (2 * wl["H"] * ((wl["W"] + 7) // 8) / 64),
                              source="SQ_INSTS_VALU of leaf_hash_kernel measured in this run (rocprofv3 --pmc pass of tools/leaf_hash_once.py); issue cost "
                                     "from profiles/r02_microbench_opcodes.txt via profiles/r02_valu_model.json")
                if vm and vm.get("valu_instr_per_perm") and vm.get("cycles_per_wave_instr"):
                    wave_instr = perms * vm["valu_instr_per_perm"] / 64
                    peak = 1024 * 2.4e9 / vm["cycles_per_wave_instr"]  # SIMDs x clock / measured cycles per wave instruction of this mix
                    rate = wave_instr / (ms / args.steps * 1e-3)
                    roof["valu"] = dict(permutations_per_step=perms, valu_instr_per_perm=vm["valu_instr_per_perm"],
                                        cycles_per_wave_instr=vm["cycles_per_wave_instr"],
                                        achieved_G_wave_instr_s=rate / 1e9, peak_G_wave_instr_s=peak / 1e9, frac=rate / peak,
                                        source=(vm.get("source", "") if live else "profiles/r02_valu_model.json: " + vm.get("source", "")),
                                        mfma="utilisation 0 by design; measured alternative in profiles/r02_microbench_mfma_mds.txt")
                else:
                    roof["valu"] = None
        by_kernel = {}
        for k, ms in stage_ms.items():
            if k in algo_bytes_per_cell and ms > 0:
                gbs = algo_bytes_per_cell[k] * cells_per_step * (committed_scale if k in per_committed else 1.0) / (ms * 1e-3) / 1e9
                rec = dict(ms=ms, algorithmic_GBps=gbs, frac_of_peak=gbs / HBM_PEAK_GBS)
                tb = traffic_db.get(k, traffic_db.get(k.split("<")[0]))
                if tb:
                    rec["pmc_traffic_bytes"] = tb
                    rec["pmc_GBps"] = tb / (ms * 1e-3) / 1e9
                by_kernel[k] = rec
        cpu = None
        if not args.no_cpu_baseline and world == 1:  # the contract: rank 0 at N = 1 only
            try:
                # (the LogUp proof commits 2.7x the columns: half the rows keep the sample at ~20 s)
                cpu = cpu_baseline(args.shape, min(args.cpu_log_height - (1 if args.logup else 0), log_h), args.queries, args.pow_bits, seed=0, logup=args.logup)
            except Exception as e:  # the baseline must never take the product number down
                cpu = dict(value=None, unit="cells/s", cores=os.cpu_count(), kind="port", sample=f"failed: {e}")
        line = dict(
            metric="STARK cells/sec (trace rows x cols) proving guest-keccak" + (" [proof includes the AIR's bus interactions (LogUp); `constraints_only` = without them]"
                                                                                     if args.logup else " [constraints-only proof; `logup` = with the bus argument]"),
            metric_short="STARK cells/sec (trace rows x cols) proving guest-keccak" + (" [bus interactions (LogUp) inside the proof]" if args.logup else " [constraints-only proof]"),
            value=value, unit="cells/s",
            n_gpus=world, steps=args.steps, warmup=args.warmup, ms_per_step=elapsed / args.steps * 1e3,
            higher_is_better=True, scaling="weak", vs_baseline=None, dtype="u32 (BabyBear, Montgomery)", data="synthetic",
            rccl_ranks=comm_facts(world)["ranks"], comm=comm_facts(world), per_rank_ms=per_rank_ms,
            strong_scaling_value=(segment_leg or {}).get("value"),
            strong_scaling_note="`value` = weak scaling (one C2 segment per rank per step); `multi_segment.value` (= strong_scaling_value) = strong scaling: "
                                "a fixed number of C4 segments placed on the ranks by cells — the >= 6x at 8 GPUs target of north_star is read off that one",
            config=dict(workload=f"{args.shape} {shape.name} autoprecompile AIR: {wl['W']} cols x 2^{log_h} rows, "
                                 f"{len(wl['cons'][1])} constraints, {wl['apc'].n_bus} bus interactions; trace generation + "
                                 f"pw-stark v0 proof (blow-up 2, {args.queries} queries, {args.pow_bits} PoW bits)"
                                 + (f" WITH the LogUp phase: {perm_cols // 4 - 1} interaction groups = {perm_cols} extra committed "
                                    f"columns, rho = {perm_cols / wl['W']:.2f} (SURVEY 8d: algorithmic bytes per main cell "
                                    f"= 48 + 4 + 44*rho = {52 + 44 * perm_cols / wl['W']:.0f})" if args.logup else
                                    "; CONSTRAINTS-ONLY proof (the bus interactions are replayed into the periphery histograms but are not "
                                    "inside this proof — see `logup` for the same step with them)")
                                 + (f"; {wl['calls']} APC calls, the remaining rows are zero padding" if wl["calls"] != wl["H"] else "")
                                 + "; one segment per step per GPU"
                                 + ("; source heights b*calls (not padded to a power of two)" if args.exact_source_heights else ""),
                        workload_short=f"{args.shape} {shape.name} APC AIR {wl['W']} cols x 2^{log_h} rows, {len(wl['cons'][1])} constraints, {wl['apc'].n_bus} bus "
                                       f"interactions; tracegen + proof" + (f" +LogUp ({perm_cols} perm cols)" if args.logup else " (constraints only)"),
                        rows=wl["H"], cols=wl["W"], perm_cols=perm_cols, parallelism=f"segments x{world}" + (f", {args.pipeline} streams per GPU" if args.pipeline > 1 else ""),
                        source_bytes=wl["src_bytes"], proof_bytes=proof_bytes, prover_device_bytes=prover_bytes,
                        caveat="proof system pw-stark v0 is this repository's own (oracle/stark_oracle.cpp); its Poseidon2 round constants are a "
                               "documented placeholder stream: proofs are byte-exact against the oracle, not interoperable with the reference prover"),
            roofline=roof, roofline_by_kernel=by_kernel, logup=logup_leg, constraints_only=constraints_only_leg, multi_segment=segment_leg, c3=c3, build=build_info(), tracegen_callmajor=callmajor_leg, tracegen_column_structured=colstruct_leg, tracegen_from_records=records_leg, cpu_baseline=cpu, stage_ms=stage_ms, gauges=gauges,
            hbm_copy_GBps_measured=copy_gbs, jit_cache=jit_cache,
        )
        emit(line)
    if world > 1:
        import torch.distributed as dist

        barrier()  # rank 0 ran the single-GPU extras (C3, checks) alone: everybody leaves together
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
