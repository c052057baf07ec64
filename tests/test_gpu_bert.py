"""BERT receive on the GPU (the "bert" option): decode of type-4 frames and the PRBS9 checker, held byte for byte to
the oracle's records with the BERT fields of tests/bert_ref.py patched in, and to the model's counters and state."""
import functools

import numpy as np
import pytest

from tests import bert_ref, oracle

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@functools.lru_cache(maxsize=None)
def _bert_sig(C, nblk, ebn0, nf=12, seed=0xBE470000):
    import m17_sdr_amd as m
    # noise band-limited to a 12.5 kHz channel, as scripts/ber_sweep.py has it (white over 48 kHz, nothing locks below ~17 dB)
    return m.generate_bert_batch(C, nblk, n_bert_frames=nf, ebn0_db=ebn0, base_seed=seed, noise_cutoff_hz=6250.0, nthreads=16)


@functools.lru_cache(maxsize=None)
def _expected(C, nblk, calls, ebn0, nf=12, sample=None):
    """oracle records per call with the BERT fields patched in (for the sampled channels), model counters and state"""
    sig = _bert_sig(C, nblk * calls, ebn0, nf)
    och = oracle.Channels(C)
    model = bert_ref.ChainModel(C)
    chans = None if sample is None else list(sample)
    out = []
    for k in range(calls):
        part = np.ascontiguousarray(sig["iq"][:, k * nblk:(k + 1) * nblk])
        ref = och.rx_blocks(part, mode=1, nthreads=16)
        out.append((ref["counts"], model.call(ref, chans)))
    return out, model.counters(), model.states()


def _run_chain(C, nblk, calls, ebn0, options, nf=12):
    torch = _torch()
    import m17_sdr_amd as m
    sig = _bert_sig(C, nblk * calls, ebn0, nf)
    rx = m.Receiver(C, nblk)
    for k, v in options.items():
        rx.set_option(k, v)
    got = []
    for k in range(calls):
        part = np.ascontiguousarray(sig["iq"][:, k * nblk:(k + 1) * nblk])
        o = rx.rx_blocks(torch.from_numpy(part).cuda(), 1, rx.alloc_outputs(nblk))
        torch.cuda.synchronize()
        got.append((o["counts"].cpu().numpy(), o["recs"].cpu().numpy().view(oracle.REC_DTYPE).reshape(C, -1)))
    return got, rx.bert(), rx


def _cmp_recs(got, want_counts, want_recs, chans):
    counts, recs = got
    np.testing.assert_array_equal(counts, want_counts)
    for c in chans:
        n = min(int(counts[c]), recs.shape[1])
        assert recs[c, :n].tobytes() == want_recs[c, :n].tobytes(), f"channel {c}: records differ"


def _cmp_bert(b, cnt, stt, chans):
    keys = ("bits", "errors", "frames", "erased", "locks", "losses")
    for i, k in enumerate(keys):
        np.testing.assert_array_equal(b[k][chans], cnt[chans, i], err_msg=k)
    for i, k in enumerate(("idx", "state", "bad", "good", "eq_cnt", "dif_cnt")):
        np.testing.assert_array_equal(b[k][chans], stt[chans, i], err_msg=k)


def test_option_off_bert_traffic_is_unchanged():
    torch = _torch()
    import m17_sdr_amd as m
    C, nblk = 256, 24
    sig = _bert_sig(C, nblk, 200.0)
    rx = m.Receiver(C, nblk)
    o = rx.rx_blocks(torch.from_numpy(sig["iq"]).cuda(), 1, rx.alloc_outputs(nblk))
    torch.cuda.synchronize()
    ref = oracle.Channels(C).rx_blocks(sig["iq"], mode=1, nthreads=16)
    recs = o["recs"].cpu().numpy().view(oracle.REC_DTYPE).reshape(C, -1)
    _cmp_recs((o["counts"].cpu().numpy(), recs), ref["counts"], ref["recs"], range(C))
    assert ((ref["recs"]["type"] == 4) & ((ref["recs"]["flags"] & 0x2) != 0)).sum() > 1000
    b = rx.bert()
    assert all(int(np.abs(v.astype(np.int64)).sum()) == 0 for v in b.values())


def test_decode_frames_stage_entry():
    torch = _torch()
    import m17_sdr_amd as m
    C, nblk = 640, 24
    sig = _bert_sig(C, nblk, 12.0)
    ref = oracle.Channels(C).rx_blocks(sig["iq"], mode=1, nthreads=16)
    frames = []
    for c in range(C):
        ns = ref["nsyms"][c]
        starts = np.concatenate([[0], np.cumsum(ns)[:-1]])
        for r in ref["recs"][c, :ref["counts"][c]]:
            if r["type"] == 4 and r["flags"] & 0x2:
                end = int(starts[r["block"]]) + int(r["sym_pos"])
                if end >= 191:
                    frames.append(ref["syms"][c, end - 191:end + 1])
    assert len(frames) >= 4096
    frames = np.array(frames[:4096], np.float32)
    rx = m.Receiver(8, 4)
    rx.set_option("bert", 1)
    got = rx.decode_frames(torch.from_numpy(frames).cuda(), torch.full((len(frames),), 4, dtype=torch.uint8).cuda())
    got = got.cpu().numpy().view(oracle.REC_DTYPE).reshape(-1)
    want = np.array([bert_ref.decode_frame(f) for f in frames])
    np.testing.assert_array_equal(got["data"][:, :25], want)
    assert not got["data"][:, 25:].any() and (got["type"] == 4).all() and not got["fn"].any()
    assert (want[:, 24] & 7 == 0).all()
    # option off: BERT frames are not decoded (their records stay as the stage entry cleared them)
    rx.set_option("bert", 0)
    off = rx.decode_frames(torch.from_numpy(frames[:64]).cuda(), torch.full((64,), 4, dtype=torch.uint8).cuda())
    assert not off.cpu().numpy().any()


def _pack(bits197):
    return np.packbits(np.asarray(bits197, np.uint8))


def test_bert_feed_stage_entry():
    torch = _torch()
    import m17_sdr_amd as m
    C, n = 256, 40
    rng = np.random.default_rng(0xB17)
    bits = np.zeros((C, n, 25), np.uint8)
    kinds = np.zeros((C, n), np.uint8)
    for c in range(C):
        idx = int(rng.integers(0, 511))                      # random start phase
        for i in range(n):
            seq = bert_ref.PRBS[(idx + np.arange(197)) % 511].copy()
            idx = (idx + 197) % 511
            kind = c % 8
            if kind == 1 and i % 7 == 3:                      # mismatch bursts of 17, 18 and 40
                L = (17, 18, 40)[i % 3]
                p = int(rng.integers(0, 197 - L))
                seq[p:p + L] ^= 1
            elif kind == 2 and i % 5 == 2:                    # random frames
                seq = rng.integers(0, 2, 197).astype(np.uint8)
            elif kind == 3 and i % 6 == 4:                    # erased frames, in sync or not
                kinds[c, i] = 1
            elif kind == 4 and i in (1, 9, 17):
                kinds[c, i] = 1
            elif kind == 5 and i in (12, 30):                 # AOS in the middle of sync, the PRBS restarting
                kinds[c, i] = 2
                idx = 0
                continue
            elif kind == 6:                                   # sparse random bit errors
                seq ^= (rng.random(197) < 0.02).astype(np.uint8)
            elif kind == 7 and i % 4 == 0:                    # bursts straddling a frame boundary
                seq[-10:] ^= 1
            bits[c, i] = _pack(seq)
    rx = m.Receiver(C, 4)
    rx.set_option("bert", 1)
    out = np.concatenate([rx.bert_feed(torch.from_numpy(np.ascontiguousarray(bits[:, k:k + 20])).cuda(),
                                       torch.from_numpy(np.ascontiguousarray(kinds[:, k:k + 20])).cuda()).cpu().numpy()
                          for k in (0, 20)], axis=1)
    want = np.zeros((C, n, 2), np.uint8)
    cks = [bert_ref.Checker() for _ in range(C)]
    for c in range(C):
        for i in range(n):
            if kinds[c, i] == 2:
                cks[c].aos()
            elif kinds[c, i] == 1:
                cks[c].erased()
            else:
                want[c, i] = cks[c].frame(bert_ref.unpack(bits[c, i]))
    np.testing.assert_array_equal(out, want)
    cnt = np.array([ck.cnt for ck in cks], np.uint64)
    stt = np.array([ck.state_row() for ck in cks], np.int32)
    _cmp_bert(rx.bert(), cnt, stt, np.arange(C))
    assert cnt[:, 5].sum() > 0 and cnt[:, 3].sum() > 0 and cnt[:, 1].sum() > 0


# (below ~8 dB on this channel the framer hardly locks on BERT traffic: at 5 and 3 dB nearly nothing is decoded, and the
#  points hold only that nothing goes wrong there)
@pytest.mark.parametrize("ebn0", [200.0, 12.0, 8.0, 5.0, 3.0])
def test_full_chain(ebn0):
    C, nblk, calls = 512, 16, 3
    exp, cnt, stt = _expected(C, nblk, calls, ebn0)
    got, b, _ = _run_chain(C, nblk, calls, ebn0, {"bert": 1})
    for k in range(calls):
        _cmp_recs(got[k], exp[k][0], exp[k][1], range(C))
    _cmp_bert(b, cnt, stt, np.arange(C))
    assert cnt[:, 2].sum() > 0
    if ebn0 >= 100:
        assert cnt[:, 4].sum() >= C                       # every channel locks
    if 5.0 < ebn0 <= 12.0:
        assert cnt[:, 1].sum() > 0


def test_noiseless_bit_counts_carry_eq_over_aos():
    """m17_prbs9_rx_reset keeps eq_cnt (m17_prbs9.cpp:36-39): a channel's first transmission hunts 18 bits, so its complete
    transmissions check 197 n - 18 bits; one behind a transmission without errors -- eq_cnt >= 197 carried over the AOS --
    locks on its first bit and checks 197 n - 1."""
    C, nblk, calls, nf = 512, 16, 3, 12
    got, _, _ = _run_chain(C, nblk, calls, 200.0, {"bert": 1})
    seen = {"first": 0, "after_clean": 0}
    for c in range(C):
        recs = np.concatenate([g[1][c, :min(int(g[0][c]), g[1].shape[1])] for g in got])
        aos = list(np.flatnonzero(recs["flags"] & 0x100)) + [len(recs)]
        prev_clean = None                                 # None: no transmission yet since reset
        for a, b in zip(aos[:-1], aos[1:]):
            seg = recs[a + 1:b]
            parsed = seg[(seg["flags"] & 0x2) != 0]
            frames = parsed[parsed["type"] == 4]
            complete = len(parsed) == nf and len(frames) == nf and ((seg["flags"] & 0x10) != 0).any()
            if complete:
                checked = int(frames["data"][:, 25].sum())
                if prev_clean is None:
                    assert checked == 197 * nf - 18, f"channel {c}: first transmission checked {checked}"
                    seen["first"] += 1
                elif prev_clean:
                    assert checked == 197 * nf - 1, f"channel {c}: transmission after a clean one checked {checked}"
                    seen["after_clean"] += 1
                prev_clean = not frames["data"][:, 26].any()
            else:
                prev_clean = False if prev_clean is not None or len(frames) else None
    assert seen["first"] > C // 4 and seen["after_clean"] > 0, seen


_PATHS = [(f, s, k) for f in (0, 1, 4, 5) for s in (0, 1, 2) for k in (0, 1, 2)]


@pytest.mark.parametrize("fir,slot,book", _PATHS)
def test_paths(fir, slot, book):
    C, nblk, calls = 64, 12, 2
    exp, cnt, stt = _expected(C, nblk, calls, 12.0)
    got, b, rx = _run_chain(C, nblk, calls, 12.0, {"bert": 1, "fir_impl": fir, "slot_impl": slot, "book_impl": book})
    for k in range(calls):
        _cmp_recs(got[k], exp[k][0], exp[k][1], range(C))
    _cmp_bert(b, cnt, stt, np.arange(C))


def test_production_size():
    C, nblk, calls = 16384, 16, 2
    sample = tuple(range(0, C, C // 512))
    exp, cnt, stt = _expected(C, nblk, calls, 12.0, 12, sample)
    got, b, _ = _run_chain(C, nblk, calls, 12.0, {"bert": 1})
    for k in range(calls):
        counts, recs = got[k]
        np.testing.assert_array_equal(counts, exp[k][0])
        want = exp[k][1]
        s = np.array(sample)
        # every record: the oracle's bytes outside the BERT fields; the sampled channels in full
        strip = recs.copy()
        wstrip = want.copy()
        for arr in (strip, wstrip):
            is_b = (arr["type"] == 4) & ((arr["flags"] & 0x2) != 0)
            arr["data"][is_b] = 0
            arr["flags"] &= ~np.uint16(bert_ref.F_BERT_SYNC)
        for c in range(C):
            n = min(int(counts[c]), recs.shape[1])
            assert strip[c, :n].tobytes() == wstrip[c, :n].tobytes(), f"channel {c}"
        _cmp_recs(got[k], exp[k][0], want, s)
    _cmp_bert(b, cnt, stt, np.array(sample))


def test_option_on_stream_traffic_is_unchanged():
    torch = _torch()
    import m17_sdr_amd as m
    C, nblk = 256, 24
    sig = m.generate_batch(C, nblk, n_stream_frames=8, ebn0_db=8.0)
    rx = m.Receiver(C, nblk)
    rx.set_option("bert", 1)
    o = rx.rx_blocks(torch.from_numpy(sig["iq"]).cuda(), 1, rx.alloc_outputs(nblk))
    torch.cuda.synchronize()
    ref = oracle.Channels(C).rx_blocks(sig["iq"], mode=1, nthreads=16)
    recs = o["recs"].cpu().numpy().view(oracle.REC_DTYPE).reshape(C, -1)
    _cmp_recs((o["counts"].cpu().numpy(), recs), ref["counts"], ref["recs"], range(C))
    b = rx.bert()
    assert all(int(v.astype(np.int64).sum()) == 0 for v in b.values())
