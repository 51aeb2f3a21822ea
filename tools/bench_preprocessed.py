"""What the preprocessed periphery layout costs: a C4 HonestSegment proven with the periphery tables in main columns ("main", the
default) and in preprocessed columns ("preprocessed"), both in this process, the two layouts alternating after a
warm-up. A step = trace generation + the segment proof; the host clock stops after a device synchronise. Prints one JSON object:
ms per segment (median and spread per layout), proof words and main-trace cells per layout.

  python tools/bench_preprocessed.py [--max-log-height 18] [--steps 6] [--warmup 2] [--out profiles/...json]"""
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
    ap.add_argument("--max-log-height", type=int, default=18)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--pow-bits", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_preprocessed: needs a GPU")
    from powdr_amd import segment_workload as sw

    layouts = ("main", "preprocessed")
    segs = {lay: sw.HonestSegment("C4", max_log_height=args.max_log_height, seed=0, queries=args.queries, pow_bits=args.pow_bits,
                                  logup=True, specialise_all=True, periphery_layout=lay) for lay in layouts}
    times = {lay: [] for lay in layouts}
    words = {}
    for it in range(args.warmup + args.steps):
        for lay in (layouts if it % 2 == 0 else layouts[::-1]):
            seg = segs[lay]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seg.generate_traces()
            pf = seg.prove(copy=False)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if it >= args.warmup:
                times[lay].append(dt * 1e3)
            words[lay] = len(pf)
    checks = {}
    for lay in layouts:
        seg = segs[lay]
        seg.generate_traces()
        checks[lay] = seg.verify(seg.prove(copy=True))
    out = dict(kind="C4", max_log_height=args.max_log_height, queries=args.queries, pow_bits=args.pow_bits, steps=args.steps,
               warmup=args.warmup, device=torch.cuda.get_device_name(0), verify=checks, layouts={})
    for lay in layouts:
        ts = times[lay]
        out["layouts"][lay] = dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
                                   ms_all=[round(t, 3) for t in ts], proof_words=words[lay], proof_bytes=4 * words[lay],
                                   main_cells=segs[lay].cells, periphery_main_cells=segs[lay].cells_by_role["periphery"],
                                   device_bytes=segs[lay].device_bytes())
    m, p = out["layouts"]["main"], out["layouts"]["preprocessed"]
    out["delta"] = dict(ms_median=round(p["ms_median"] - m["ms_median"], 3), proof_words=p["proof_words"] - m["proof_words"],
                        main_cells=p["main_cells"] - m["main_cells"], device_bytes=p["device_bytes"] - m["device_bytes"])
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    for seg in segs.values():
        seg.close()


if __name__ == "__main__":
    main()
