"""The Poseidon2 compression chip (pw_poseidon2_compress_trace, system_airs.poseidon2_air): what its trace generator and
its proof cost. A new capability has no parent figure, so the generator is reported against two yardsticks of the same build:
  (a) prove_segment of the same segment (a hash-user AIR that sends every request, and the chip);
  (b) permutations per second of compress_rows_kernel against compress_kernel (the Merkle kernel: the same arithmetic without the
      1.2 KB of stores per row) on a tree whose compress_kernel launches make 2^k - 2^11 permutations for the chip's 2^k rows.
The proof of the chip alone (a one-AIR segment) is reported interpreted (POWDR_JIT=0) against specialised (POWDR_JIT=1): 290 wide
constraints are a new shape for both paths. One process, the measurements alternating after a warm-up, host clock around calls that
synchronise themselves; kernel times from the library's HIP events. Sizes: 2^log distinct requests for every --log-requests, without
duplicates and with every request sent twice (50 % duplicates). The senders' digests are copied from the chip's own trace (after the
bus check has confirmed nothing: they are then right by construction, and check_segment_buses must say so). Prints one JSON object and
writes it to --out.

  python tools/bench_poseidon2_air.py [--log-requests 16 20] [--steps 3] [--warmup 1] [--generator-only] [--out profiles/poseidon2_air.json]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-requests", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--generator-only", action="store_true", help="no proofs (the run a kernel trace is taken of)")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "poseidon2_air.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_poseidon2_air: needs a GPU")
    from powdr_amd import abi, prover
    from powdr_amd import system_airs as sa
    from tests import _poseidon2_air_ref as ref

    note = lambda *a: print("[bench_poseidon2_air]", *a, file=sys.stderr, flush=True)
    no_cons = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))
    W, P, BUS = sa.POSEIDON2_WIDTH, sa.P, sa.BUS_COMPRESS

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ts):
        return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), ms_all=[round(t, 3) for t in ts])

    def events(fn, prefixes):
        abi.lib.powdr_gpu_timing_enable(1)
        fn()
        torch.cuda.synchronize()
        kern = {k: dict(launches=v[0], ms=round(v[1], 4)) for k, v in abi.timing_report().items() if k.startswith(prefixes)}
        abi.lib.powdr_gpu_timing_enable(0)
        return kern

    def with_jit(mode, fn):
        def run():
            os.environ["POWDR_JIT"] = mode
            try:
                return fn()
            finally:
                os.environ.pop("POWDR_JIT", None)
        return run

    air = sa.poseidon2_air()
    user_it = ref.hash_user_interactions(BUS)
    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, queries=args.queries, cases={})
    for lg in args.log_requests:
        for dup in (False, True):
            name = f"2^{lg}_distinct" + ("_each_sent_twice" if dup else "")
            n, lh_user = 1 << lg, lg + (1 if dup else 0)
            rows_user = 1 << lh_user
            # the sender on the device: is_valid = 1, 16 random words per row below p (Montgomery words of SOME values), digests later
            g = torch.Generator(device="cuda").manual_seed(lg)
            user = torch.zeros((ref.USER_WIDTH, rows_user), dtype=torch.int32, device="cuda")
            user[0] = 0x0ffffffe  # Montgomery 1
            user[1:17, :n] = torch.randint(0, P, (16, n), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
            if dup:
                user[1:17, n:] = user[1:17, :n]
            p_user = prover.Prover(ref.USER_WIDTH, *no_cons, num_queries=args.queries, interactions=user_it)
            senders = [(p_user, user.data_ptr(), lh_user)]
            out = torch.empty(W << lg, dtype=torch.int32, device="cuda")
            gen = lambda: sa.poseidon2_compress_trace(senders, lg, out=out)
            trace, lh, rows, status = gen()
            assert (lh, rows, status) == (lg, n, 0)
            table = sa.last_stats()
            # the digests the chip computed are what an honest sender sends: rows are in witness order = the sender's row order
            digests = trace.view(W, n)[sa.P2_OUT:sa.P2_OUT + 8]
            user[17:25, :n] = digests
            if dup:
                user[17:25, n:] = digests
            p_chip = {m: air.make_prover(args.queries) for m in (("0",) if args.generator_only else ("0", "1"))}
            seg = lambda m: senders + [(p_chip[m], trace.data_ptr(), lg)]
            summaries, tuples = prover.check_segment_buses(seg("0"), buses=[BUS])
            assert summaries[0]["status"] == 0 and summaries[0]["n_active"] == rows_user + n and not tuples
            runs = {"poseidon2_compress_trace": gen}
            if not args.generator_only:
                assert p_chip["0"].check_constraints(trace.data_ptr(), lg) == (0, None, None)
                runs["prove_segment_sender_and_chip"] = with_jit("0", lambda: prover.prove_segment(seg("0"), logup=True, copy=False))
                if not dup:
                    runs["prove_chip_interpreted"] = with_jit("0", lambda: prover.prove_segment([seg("0")[-1]], logup=True, copy=False))
                    t0 = time.perf_counter()
                    with_jit("1", p_chip["1"].specialise)()
                    compile_s = round(time.perf_counter() - t0, 2)
                    runs["prove_chip_specialised"] = with_jit("1", lambda: prover.prove_segment([seg("1")[-1]], logup=True, copy=False))
            times = {k: [] for k in runs}
            for it in range(args.warmup + args.steps):
                for k in (list(runs) if it % 2 == 0 else list(runs)[::-1]):
                    dt, _ = timed(runs[k])
                    if it >= args.warmup:
                        times[k].append(dt)
                    note(name, it, k, round(dt, 2), "ms")
            case = dict(distinct_requests=n, requests=rows_user, chip_log_height=lg, runs={k: stats(v) for k, v in times.items()}, table=table,
                        kernels_event_timed=events(gen, ("compress_",)))
            rk = case["kernels_event_timed"]["compress_rows_kernel"]["ms"]
            case["compress_rows_kernel_permutations_per_second"] = round(n / (rk * 1e-3))
            case["compress_rows_kernel_store_GB_per_second"] = round(n * W * 4 / (rk * 1e-3) / 1e9, 1)
            # yardstick (b): the Merkle tree of 2^lg leaves: its compress_kernel launches (levels above 2048 nodes) make 2^lg - 2^11 permutations
            leaves = torch.zeros(8 << lg, dtype=torch.int32, device="cuda")
            digs = torch.empty(((2 << lg) - 1) * 8, dtype=torch.int32, device="cuda")
            commit = lambda: abi.check(prover.lib.pw_merkle_commit(leaves.data_ptr(), n, 8, digs.data_ptr()), "pw_merkle_commit")
            commit()
            ck = events(commit, ("compress_kernel",))["compress_kernel"]
            perms = n - 2048
            case["compress_kernel"] = dict(ck, permutations=perms, permutations_per_second=round(perms / (ck["ms"] * 1e-3)))
            case["yardstick_b_rows_kernel_over_compress_kernel_time_per_permutation"] = round((rk / n) / (ck["ms"] / perms), 3)
            if "prove_segment_sender_and_chip" in case["runs"]:
                case["yardstick_a_generator_over_prove_segment"] = round(case["runs"]["poseidon2_compress_trace"]["ms_median"]
                                                                         / case["runs"]["prove_segment_sender_and_chip"]["ms_median"], 4)
            if "prove_chip_specialised" in case["runs"]:
                case["chip_proof_interpreted_over_specialised"] = round(case["runs"]["prove_chip_interpreted"]["ms_median"]
                                                                        / case["runs"]["prove_chip_specialised"]["ms_median"], 3)
                case["specialise_seconds_first_time"] = compile_s
                case["specialised"] = p_chip["1"].specialised()
            result["cases"][name] = case
            for p in list(p_chip.values()) + [p_user]:
                p.close()
            del user, out, trace, digests, leaves, digs
            torch.cuda.empty_cache()
    result["not_measured"] = ["the interpreter path of the senders' interactions (POWDR_LOGUP_INTERPRET=1)", "senders with more than one interaction on the bus",
                              "hardware counters of compress_rows_kernel (VALU busy, write traffic): the bound named in DESIGN.md §5l is an inference from the two rates",
                              "yardstick (b) compares against the tree's compress_kernel launches, which shrink level by level (2^k-1 ... 2^11 parents), not one launch of 2^k",
                              "a build of the parent: the capability does not exist there"]
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
