#!/usr/bin/env python3
"""Step time of the full chain with BERT receive, at 16,384 channels x 16 blocks:
  (a) stream traffic, option "bert" off;  (b) stream traffic, option on;  (c) BERT traffic, option on.
Each case: its own receiver, one 16-block slab fed back to back (untimed settle, warm-up), then K timed steps between HIP
events on the receiver's stream; the checker kernel's share comes from a rocprofv3 --kernel-trace --stats pass (--case c).

    python scripts/bench_bert.py --out profiles/bert_step_times.json
    rocprofv3 --kernel-trace --stats -d DIR -o bert -- python scripts/bench_bert.py --case c --steps 20"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_case(torch, m, C, nblk, traffic, bert, steps, warmup, settle_s=0.4):
    rx = m.Receiver(C, nblk)
    rx.set_option("bert", bert)
    if traffic == "stream":
        iq = rx.gen_batch(nblk, n_stream_frames=nblk)["iq"]
    else:
        iq = torch.from_numpy(m.generate_bert_batch(C, nblk, n_bert_frames=12, nthreads=16)["iq"]).cuda()
    out = rx.alloc_outputs(nblk)
    t0 = time.time()
    settled = 0
    while time.time() - t0 < settle_s:
        rx.rx_blocks(iq, 1, out)
        torch.cuda.synchronize()
        settled += 1
    rx.reset()
    for _ in range(warmup):
        rx.rx_blocks(iq, 1, out)
    s = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record(s)
    for k in range(steps):
        rx.rx_blocks(iq, 1, out)
        ev[k + 1].record(s)
    torch.cuda.synchronize()
    ms = [ev[k].elapsed_time(ev[k + 1]) for k in range(steps)]
    b = rx.bert()
    return {"traffic": traffic, "bert": bert, "ms_per_step": float(np.mean(ms)), "ms_median": float(np.median(ms)),
            "ms_min": float(np.min(ms)), "steps": steps, "warmup": warmup, "settle_calls": settled,
            "bert_frames": int(b["frames"].sum()), "bits_in_sync": int(b["bits"].sum()), "errors": int(b["errors"].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=16384)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--case", choices=["a", "b", "c", "all"], default="all")
    ap.add_argument("--rounds", type=int, default=2, help="a, b, c in turn this many times (--case all)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import m17_sdr_amd as m
    cases = {"a": ("stream", 0), "b": ("stream", 1), "c": ("bert", 1)}
    order = ["a", "b", "c"] * a.rounds if a.case == "all" else [a.case]
    rows = []
    for k in order:
        r = time_case(torch, m, a.channels, a.blocks, *cases[k], a.steps, a.warmup)
        r["case"] = k
        rows.append(r)
        print(json.dumps(r), flush=True)
    res = {"channels": a.channels, "blocks": a.blocks, "rows": rows}
    if a.case == "all":
        best = {k: min(r["ms_per_step"] for r in rows if r["case"] == k) for k in "abc"}
        res["best_ms"] = best
        res["b_over_a"] = best["b"] / best["a"] - 1.0
        res["c_over_a"] = best["c"] / best["a"] - 1.0
        print(json.dumps({"best_ms": best, "b_over_a": res["b_over_a"], "c_over_a": res["c_over_a"]}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
