"""The device memory the provers plan and hold, for a fixed list of AIRs: the figures that must not move when the per-AIR buffer
plan is refactored (csrc/prover_stages.hpp plan_stage_buffers). Run it on two trees and compare the outputs.

  one_air   constraints-only and LogUp provers (the kinds pw_prover_prove accepts) at 2^12, 2^16 and 2^20 rows, in fresh processes
            with POWDR_STREAM_LOG_BLOCKS = 0, 1, 2: device_bytes() after reserve(), stream_log_blocks[_consuming]()
  segment   one LogUp segment of four AIRs — constraints-only, LogUp, preprocessed, row-aware — proven once in a fresh process under a
            budget nothing is streamed for, and once under 60 % of the resident plan: segment_last_plan(), segment_last_plan_tables(),
            segment_last_modes(), segment_context_bytes() and every prover's device_bytes()

The budget is always set (64 GiB in the first case), so that what the policy has to work with does not depend on what else runs on
the device. The traces are random: the proofs are not meant to verify. Prints one JSON object.

  python tools/stage_sharing_memory.py [--out profiles/stage_sharing_memory.json]"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

W, PRE_W, N_CONS, N_INTER = 512, 8, 32, 6  # (wide enough that a streamed AIR is smaller than a resident one)
PA, PC, ADD, SUB, MUL = 0, 1, 2, 3, 4
HEIGHTS = (12, 16, 20)
SEGMENT = (("constraints", 16), ("logup", 18), ("preprocessed", 12), ("row_aware", 14))  # (kind, log_height)
ROOMY = 64 << 30


def tables(progs):
    bc, sp = [], []
    for p in progs:
        sp.append((len(bc), len(p)))
        bc += p
    return np.array(bc, np.uint32), np.array(sp, np.uint32).reshape(-1, 2)


def constraints(kind: str):
    """N_CONS constraints c_a c_b - c_d + c_e; the preprocessed AIR reads fixed columns in them, the row-aware one puts a quarter of
    them under is_transition on a next-row column."""
    from powdr_amd.prover import row_operands

    rng = np.random.default_rng(3)
    cols = W + PRE_W if kind == "preprocessed" else W
    r = row_operands(W)
    progs = []
    for k in range(N_CONS):
        a, b, d, e = (int(x) for x in rng.integers(0, cols, 4))
        if kind == "row_aware" and k % 4 == 0:
            progs.append([PA, r.is_transition, PA, r.next(a), PA, b, PA, d, MUL, SUB, MUL])
        else:
            progs.append([PA, a, PA, b, MUL, PA, d, SUB, PA, e, ADD])
    return tables(progs)


def interactions(n: int):
    """n interactions of two arguments on buses 1..n: multiplicity and arguments are columns"""
    rng = np.random.default_rng(5)
    inter, progs = [], []
    for i in range(n):
        inter.append((i + 1, 2, len(progs)))
        progs += [[PA, int(c)] for c in rng.integers(0, W, 3)]
    bc, sp = tables(progs)
    return np.array(inter, np.uint32).reshape(-1, 3), sp, bc


def make_prover(kind: str, log_h: int, in_segment: bool):
    import torch

    from powdr_amd import prover

    inter = interactions(N_INTER if kind == "logup" else 0) if (in_segment or kind == "logup") else None
    pre = None
    if kind == "preprocessed":
        gen = torch.Generator(device="cuda").manual_seed(7)
        fixed = torch.randint(0, 0x78000001, (PRE_W << log_h,), device="cuda", dtype=torch.int64, generator=gen).to(torch.int32)
        pre = (fixed, PRE_W, log_h)
    return prover.Prover(W, *constraints(kind), num_queries=20, pow_bits=0, interactions=inter, preprocessed=pre, transition=kind == "row_aware")


def child_one_air():
    out = {}
    for kind in ("constraints", "logup"):
        for lh in HEIGHTS:
            p = make_prover(kind, lh, False)
            p.reserve(lh)
            out[f"{kind}@{lh}"] = dict(device_bytes=p.device_bytes(), stream_log_blocks=p.stream_log_blocks(lh),
                                       stream_log_blocks_consuming=p.stream_log_blocks_consuming(lh))
            p.close()
    return out


def child_segment(budget: int):
    import torch

    from powdr_amd import prover

    prover.set_device_budget(budget)
    airs, keep = [], []
    for kind, lh in SEGMENT:
        p = make_prover(kind, lh, True)
        gen = torch.Generator(device="cuda").manual_seed(lh)
        x = torch.randint(0, 0x78000001, (W << lh,), device="cuda", dtype=torch.int64, generator=gen)
        keep.append(((x << 32) % 0x78000001).to(torch.int32))  # Montgomery form of a canonical word
        airs.append((p, keep[-1].data_ptr(), lh))
    prover.prove_segment(airs, logup=True, copy=False)
    resident, streamed, b_max = prover.segment_last_plan_tables()
    out = dict(budget=budget, last_plan=list(prover.segment_last_plan()), plan_resident=resident, plan_streamed=streamed, plan_b_max=b_max,
               last_modes=[list(m) for m in prover.segment_last_modes()], context_bytes=prover.segment_context_bytes(),
               prover_device_bytes=[p.device_bytes() for p, _, _ in airs])
    for p, _, _ in airs:
        p.close()
    return out


def run_child(what: str, env=None):
    e = dict(os.environ)
    e.pop("POWDR_STREAM_LOG_BLOCKS", None)
    e.update(env or {})
    r = subprocess.run([sys.executable, __file__, "--child", what], env=e, capture_output=True, text=True, timeout=600)
    if r.returncode:
        sys.exit(f"stage_sharing_memory: child {what} failed ({r.returncode})\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child == "one_air":
        print(json.dumps(child_one_air()))
        return
    if args.child:
        print(json.dumps(child_segment(int(args.child))))
        return
    out = dict(width=W, pre_width=PRE_W, constraints=N_CONS, interactions=N_INTER, segment=[list(s) for s in SEGMENT], one_air={})
    for b in (0, 1, 2):
        out["one_air"][f"POWDR_STREAM_LOG_BLOCKS={b}"] = run_child("one_air", {"POWDR_STREAM_LOG_BLOCKS": str(b)})
    roomy = run_child(str(ROOMY))
    assert all(b == 0 for b, _ in roomy["last_modes"]), roomy["last_modes"]
    tight = run_child(str(roomy["last_plan"][0] * 6 // 10))
    assert any(b > 0 for b, _ in tight["last_modes"]), tight["last_modes"]
    out["segment_resident"], out["segment_streamed"] = roomy, tight
    text = json.dumps(out, indent=1) + "\n"
    print(json.dumps(out))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
