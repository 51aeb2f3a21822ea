"""What public values cost: an AIR of width 256 with 192 degree-2 constraints, 64 of which subtract a distinct public
value, against its twin with those 64 values as constants — the yardstick, on the same build: the capability has no earlier figure. Each
AIR is alone in a LogUp segment (no interactions), once with the run-time specialised kernels and once with the interpreter, the runs
alternating in this process after a warm-up, at each height. The proof time comes from HIP events around the call (which ends in a
device synchronise); one more proof per prover with the library's per-kernel event timing gives the kernels. The traces are random (the
proofs are not meant to verify: the cost does not depend on the values). By argument the values are scalar loads at wave-uniform
addresses and the ratio sits inside the twin's own run-to-run spread; where it does not, `outside_spread` names the kernel that carries
the difference. Prints one JSON object.

  python tools/bench_public_values.py [--log-heights 18 20] [--steps 5] [--warmup 2] [--paths specialised interpreted]
                                      [--out profiles/public_values.json] [--merge FILE.json ...]

--merge: JSON files whose top-level keys are copied into the record (the headline comparison with the parent commit, made by a run of
bench.py on both trees, and the list of what was not measured)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

W, N_PUB, N_PLAIN = 256, 64, 128  # columns; constraints that subtract a public value (twin: a constant); constraints shared by both
PA, PC, ADD, SUB, MUL = 0, 1, 2, 3, 4
QUOTIENT = ("quotient_kernel", "quotient_combine_kernel", "quotient_logup_kernel", "quotient_jit_kernel", "quotient_logup_jit_kernel",
            "quotient_logup_tail_kernel", "quotient_split_kernel")


def programs(public: bool):
    """N_PLAIN constraints c_a c_b - c_d + c_e; N_PUB constraints c_i c_j - pv_k (twin: - the constant 1000003 k + 17), all degree 2"""
    from powdr_amd.prover import row_operands

    r = row_operands(W)
    rng = np.random.default_rng(1)
    progs = []
    for _ in range(N_PLAIN):
        a, b, d, e = (int(x) for x in rng.integers(0, W, 4))
        progs.append([PA, a, PA, b, MUL, PA, d, SUB, PA, e, ADD])
    for k in range(N_PUB):
        i, j = (int(x) for x in rng.integers(0, W, 2))
        progs.append([PA, i, PA, j, MUL] + ([PA, r.public(k)] if public else [PC, value(k)]) + [SUB])
    bc, sp = [], []
    for p in progs:
        sp.append((len(bc), len(p)))
        bc += p
    return np.array(bc, np.uint32), np.array(sp, np.uint32).reshape(-1, 2)


def value(k: int) -> int:
    return 1000003 * k + 17


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-heights", type=int, nargs="+", default=[18, 20])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--pow-bits", type=int, default=16)
    ap.add_argument("--paths", nargs="+", default=["specialised", "interpreted"], choices=["specialised", "interpreted"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="*", default=[])
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_public_values: needs a GPU")
    from powdr_amd import abi, prover

    no_inter = (np.zeros((0, 3), np.uint32), np.zeros((0, 2), np.uint32), np.zeros(0, np.uint32))
    kinds = ("public", "twin")
    out = dict(width=W, constraints=N_PLAIN + N_PUB, public_constraints=N_PUB, public_values=N_PUB, segment="one AIR, LogUp, no interactions",
               yardstick="the twin (the 64 values as constants) on the same build", queries=args.queries, pow_bits=args.pow_bits, steps=args.steps,
               warmup=args.warmup, device=torch.cuda.get_device_name(0),
               timing="HIP events around pw_prove_segment; kernels: per-kernel HIP events of one more proof", paths={})
    for path in args.paths:
        # the interpreter: provers that are never specialised (POWDR_JIT=0 while they exist); specialised: compiled now
        if path == "interpreted":
            os.environ["POWDR_JIT"] = "0"
        provers = {k: prover.Prover(W, *programs(k == "public"), num_queries=args.queries, pow_bits=args.pow_bits, interactions=no_inter,
                                    n_public=N_PUB if k == "public" else 0) for k in kinds}
        provers["public"].set_public_values([value(k) for k in range(N_PUB)])
        assert provers["public"].max_constraint_degree() == provers["twin"].max_constraint_degree() == 2
        if path == "specialised":
            assert prover.specialise_all(list(provers.values())) == 2, "no run-time compiler: the specialised path cannot be measured"
        heights = {}
        for lh in args.log_heights:
            H = 1 << lh
            gen = torch.Generator(device="cuda").manual_seed(lh)
            x = torch.randint(0, 0x78000001, (W * H,), device="cuda", dtype=torch.int64, generator=gen)
            trace = ((x << 32) % 0x78000001).to(torch.int32)  # random canonical words < p in Montgomery form
            del x
            times = {k: [] for k in kinds}
            for it in range(args.warmup + args.steps):
                for k in (kinds if it % 2 == 0 else kinds[::-1]):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    prover.prove_segment([(provers[k], trace.data_ptr(), lh)], logup=True, copy=False)
                    e1.record()
                    torch.cuda.synchronize()
                    if it >= args.warmup:
                        times[k].append(e0.elapsed_time(e1))
            res = {}
            for k in kinds:
                abi.lib.powdr_gpu_timing_enable(1)
                prover.prove_segment([(provers[k], trace.data_ptr(), lh)], logup=True, copy=False)
                rep = abi.timing_report()
                abi.lib.powdr_gpu_timing_enable(0)
                ts = times[k]
                res[k] = dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
                              ms_all=[round(t, 3) for t in ts], kernels_ms={n: round(rep[n][1], 3) for n in sorted(rep)},
                              specialised=provers[k].specialised()["state"] == 1)
            assert res["public"]["specialised"] == res["twin"]["specialised"] == (path == "specialised")
            tw = res["twin"]
            res["ratio"] = round(res["public"]["ms_median"] / tw["ms_median"], 4)
            res["twin_spread"] = [round(tw["ms_min"] / tw["ms_median"], 4), round(tw["ms_max"] / tw["ms_median"], 4)]
            res["kernel_ratio"] = {n: round(res["public"]["kernels_ms"][n] / t, 4) for n, t in tw["kernels_ms"].items()
                                   if t > 0 and n in res["public"]["kernels_ms"]}
            res["kernel_delta_ms"] = {n: round(res["public"]["kernels_ms"].get(n, 0.0) - t, 3) for n, t in tw["kernels_ms"].items()}
            res["inside_twin_spread"] = res["twin_spread"][0] <= res["ratio"] <= res["twin_spread"][1]
            if not res["inside_twin_spread"]:
                res["outside_spread"] = dict(largest_kernel_delta=max(res["kernel_delta_ms"], key=lambda n: abs(res["kernel_delta_ms"][n])),
                                             quotient_delta_ms=round(sum(res["kernel_delta_ms"].get(n, 0.0) for n in QUOTIENT), 3))
            heights[str(lh)] = res
            del trace
            torch.cuda.empty_cache()
        out["paths"][path] = heights
        for p in provers.values():
            p.close()
        os.environ.pop("POWDR_JIT", None)
    for f in args.merge:
        out.update(json.loads(Path(f).read_text()))
    print(json.dumps(out))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
