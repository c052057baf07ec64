#!/usr/bin/env python3
"""BER measured by the receiver's own PRBS9 checker (the "bert" option) on BERT traffic: errors / bits checked in sync
at Eb/N0 0..10 dB and noiseless, 16,384 channels; GPU == restatement (tests/bert_ref.py on the oracle's records) on a
fixed sample of 512 channels at every point.  Noise band-limited to a 12.5 kHz channel as scripts/ber_sweep.py has it.

    python scripts/bert_sweep.py --out profiles/bert_sweep_16384ch.json"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=16384)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--frames", type=int, default=12, help="BERT frames per transmission")
    ap.add_argument("--ebn0", type=float, nargs="*", default=[float(x) for x in range(0, 11)] + [200.0])
    ap.add_argument("--noise-cutoff", type=float, default=6250.0)
    ap.add_argument("--sample", type=int, default=512)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import m17_sdr_amd as m
    from tests import bert_ref, oracle
    C, nblk = a.channels, a.blocks
    sample = list(range(0, C, max(1, C // a.sample)))[:a.sample]
    rows = []
    for eb in a.ebn0:
        t0 = time.time()
        sig = m.generate_bert_batch(C, nblk, n_bert_frames=a.frames, ebn0_db=eb, noise_cutoff_hz=a.noise_cutoff, nthreads=16)
        rx = m.Receiver(C, nblk)
        rx.set_option("bert", 1)
        out = rx.rx_blocks(torch.from_numpy(sig["iq"]).cuda(), 1, rx.alloc_outputs(nblk))
        torch.cuda.synchronize()
        b = rx.bert()
        recs = out["recs"].cpu().numpy().view(oracle.REC_DTYPE).reshape(C, -1)
        counts = out["counts"].cpu().numpy()
        sub = np.ascontiguousarray(sig["iq"][sample])
        ref = oracle.Channels(len(sample)).rx_blocks(sub, mode=1, nthreads=16)
        model = bert_ref.ChainModel(len(sample))
        want = model.call(ref)
        cnt, stt = model.counters(), model.states()
        same = bool(np.array_equal(ref["counts"], counts[sample]))
        for i, c in enumerate(sample):
            n = min(int(counts[c]), recs.shape[1])
            same = same and recs[c, :n].tobytes() == want[i, :n].tobytes()
        keys = ("bits", "errors", "frames", "erased", "locks", "losses")
        same = same and all(np.array_equal(b[k][sample], cnt[:, j]) for j, k in enumerate(keys))
        same = same and all(np.array_equal(b[k][sample], stt[:, j])
                            for j, k in enumerate(("idx", "state", "bad", "good", "eq_cnt", "dif_cnt")))
        bits, errs = int(b["bits"].sum()), int(b["errors"].sum())
        row = {"ebn0_db": eb, "bits_in_sync": bits, "errors": errs, "ber": errs / bits if bits else None,
               "bert_frames_decoded": int(b["frames"].sum()), "bert_frames_sent": int(sig["nframes"].sum()),
               "erased": int(b["erased"].sum()), "locks": int(b["locks"].sum()), "losses": int(b["losses"].sum()),
               "gpu_equals_restatement_on_sample": same, "sample_channels": len(sample), "s": round(time.time() - t0, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del rx
    res = {"channels": C, "blocks": nblk, "frames_per_transmission": a.frames, "noise_cutoff_hz": a.noise_cutoff,
           "axis": "ebn0_db of the generator: energy per channel bit over N0 (scripts/ber_sweep.py)", "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    assert all(r["gpu_equals_restatement_on_sample"] for r in rows), "GPU differs from the restatement"


if __name__ == "__main__":
    main()
