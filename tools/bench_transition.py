"""What the row layout costs: a row-aware AIR of width 256 — a third of its constraints under is_transition, reading
next rows — against a plain twin of the same width, constraint count and degrees, each proven alone in a LogUp segment (no
interactions), the two alternating in this process after a warm-up, at each height. The proof time comes from HIP events around the
call (the call ends in a device synchronise). One more proof per AIR with the library's per-kernel event timing gives the stages:
openings (weights + dot products), quotient (constraint kernels + split; the row layout's own kernel apart), DEEP. The traces are
random (the proofs are not meant to verify: the cost does not depend on the values). Prints one JSON object.

  python tools/bench_transition.py [--log-heights 18 20] [--steps 5] [--warmup 2] [--out profiles/transition_segment.json]"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

W, N_ROW, N_PLAIN = 256, 64, 128  # columns; constraints under is_transition (row-aware AIR) / their twins; constraints shared by both
PA, PC, ADD, SUB, MUL = 0, 1, 2, 3, 4
STAGES = {
    "openings": ("barycentric_weights_kernel", "zeta_weights_kernel", "ext_dot_partial_kernel"),
    "quotient": ("quotient_kernel", "quotient_combine_kernel", "quotient_logup_kernel", "quotient_jit_kernel", "quotient_logup_jit_kernel",
                 "quotient_logup_tail_kernel", "quotient_split_kernel"),
    "row_layout": ("row_layout_kernel",),
    "deep": ("deep_kernel", "deep_logup_kernel", "deep_two_point_kernel", "deep_from_combo_kernel", "ext_lincomb_kernel"),
}


def programs(row_aware: bool):
    """The same shapes in both: N_PLAIN constraints c_a c_b - c_d + c_e; N_ROW constraints is_transition (c_i' - c_j c_k) in the
    row-aware AIR, c_i - c_j c_k in the twin (degree 2 both: is_transition has degree 0)."""
    from powdr_amd.prover import row_operands

    r = row_operands(W)
    rng = np.random.default_rng(1)
    progs = []
    for _ in range(N_PLAIN):
        a, b, d, e = (int(x) for x in rng.integers(0, W, 4))
        progs.append([PA, a, PA, b, MUL, PA, d, SUB, PA, e, ADD])
    for k in range(N_ROW):
        i, j, l = 3 * k % W, int(rng.integers(0, W)), int(rng.integers(0, W))
        body = [PA, j, PA, l, MUL, SUB]
        progs.append([PA, r.is_transition, PA, r.next(i)] + body + [MUL] if row_aware else [PA, i] + body)
    bc, sp = [], []
    for p in progs:
        sp.append((len(bc), len(p)))
        bc += p
    return np.array(bc, np.uint32), np.array(sp, np.uint32).reshape(-1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-heights", type=int, nargs="+", default=[18, 20])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--pow-bits", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_transition: needs a GPU")
    from powdr_amd import abi, prover

    no_inter = (np.zeros((0, 3), np.uint32), np.zeros((0, 2), np.uint32), np.zeros(0, np.uint32))
    kinds = ("row_aware", "twin")
    provers = {k: prover.Prover(W, *programs(k == "row_aware"), num_queries=args.queries, pow_bits=args.pow_bits, interactions=no_inter,
                                transition=k == "row_aware") for k in kinds}
    assert provers["row_aware"].row_flags == 3 and provers["twin"].row_flags == 0
    assert provers["row_aware"].max_constraint_degree() == provers["twin"].max_constraint_degree() == 2
    out = dict(width=W, constraints=N_PLAIN + N_ROW, row_constraints=N_ROW, next_row_columns=N_ROW, segment="one AIR, LogUp, no interactions",
               path="as pw_prove_segment picks (the specialised kernels where hiprtc is available)", queries=args.queries, pow_bits=args.pow_bits, steps=args.steps, warmup=args.warmup,
               device=torch.cuda.get_device_name(0), timing="HIP events around pw_prove_segment; stages: per-kernel HIP events", heights={})
    for lh in args.log_heights:
        H = 1 << lh
        gen = torch.Generator(device="cuda").manual_seed(lh)
        # random canonical words < p in Montgomery form: (x 2^32) mod p
        x = torch.randint(0, 0x78000001, (W * H,), device="cuda", dtype=torch.int64, generator=gen)
        trace = ((x << 32) % 0x78000001).to(torch.int32)
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
            stages = {s: round(sum(rep[n][1] for n in names if n in rep), 3) for s, names in STAGES.items()}
            ts = times[k]
            res[k] = dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
                          ms_all=[round(t, 3) for t in ts], stages_ms=stages, quotient_kernels=sorted(n for n in rep if n in STAGES["quotient"]),
                          device_bytes=provers[k].device_bytes())
        ratio = res["row_aware"]["ms_median"] / res["twin"]["ms_median"]
        res["ratio"] = round(ratio, 4)
        res["stage_delta_ms"] = {s: round(res["row_aware"]["stages_ms"][s] - res["twin"]["stages_ms"][s], 3) for s in STAGES}
        # the row layout's memory: the next-row columns read and the selectors, N rows each, behind the AIR's LDE
        res["device_bytes_delta"] = res["row_aware"]["device_bytes"] - res["twin"]["device_bytes"]
        res["row_layout_lde_bytes"] = (N_ROW + 3) * 2 * H * 4  # (+ the three selector columns)
        out["heights"][str(lh)] = res
        del trace
        torch.cuda.empty_cache()
    top = out["heights"][str(max(args.log_heights))]
    out["target"] = dict(max_ratio=1.10, log_height=max(args.log_heights), ratio=top["ratio"], met=top["ratio"] <= 1.10)
    if not out["target"]["met"]:
        out["target"]["largest_stage_delta"] = max(top["stage_delta_ms"], key=lambda s: top["stage_delta_ms"][s])
    print(json.dumps(out))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    for p in provers.values():
        p.close()


if __name__ == "__main__":
    main()
