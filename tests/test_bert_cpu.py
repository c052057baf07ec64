"""BERT receive, CPU side: the product's BERT transmitter against the oracle's transmit primitives, the decode model
on clean frames, properties of the PRBS9 checker restatement and its feed rules (tests/bert_ref.py), and the
transmissions of m17gen_bert_batch through the oracle's receive chain."""
import ctypes as C

import numpy as np

from tests import bert_ref, oracle


def _lib():
    import m17_sdr_amd as m
    return m.lib()


def test_bert_frame_dibits_match_oracle_primitives():
    lib = _lib()
    idx = C.c_uint16(0)
    ref_idx = 0
    for f in range(8):
        d = np.zeros(192, np.uint8)
        assert lib.m17gen_bert_frame_dibits(C.byref(idx), d.ctypes.data_as(C.c_void_p)) == 192
        want, ref_idx = bert_ref.bert_frame_dibits(ref_idx)
        np.testing.assert_array_equal(d, want, err_msg=f"frame {f}")
        assert idx.value == ref_idx == (197 * (f + 1)) % 511


def _symbols(dibits):
    """ideal symbols of the dibits, at the amplitudes the demapper expects (+-1, +-3 scaled as m17_dsp.cpp:29-35)"""
    lut = np.array([1.0, 3.0, -1.0, -3.0], np.float32)          # m17_tx_routines deviation order: 0:+1 1:+3 2:-1 3:-3
    return lut[dibits]


def test_clean_frames_decode_to_the_prbs_windows():
    idx = 0
    for f in range(6):
        d, nxt = bert_ref.bert_frame_dibits(idx)
        bits = bert_ref.unpack(bert_ref.decode_frame(_symbols(d)))
        np.testing.assert_array_equal(bits, bert_ref.PRBS[(idx + np.arange(197)) % 511], err_msg=f"frame {f}")
        idx = nxt


def _seq(start, n):
    return bert_ref.PRBS[(start + np.arange(n)) % 511]


def test_checker_locks_from_every_phase_within_534_bits():
    worst = 0
    for ph in range(511):
        ck = bert_ref.Checker()
        for k, b in enumerate(_seq(ph, 600)):
            ck.bit(b)
            if ck.state == bert_ref.IN_SYNC:
                worst = max(worst, k + 1)
                break
        else:
            raise AssertionError(f"no lock from phase {ph}")
        assert ck.good == 0
    assert worst <= 534


def test_checker_good_counter_never_counts_and_errors_are_seen():
    ck = bert_ref.Checker()
    s = _seq(0, 2000).copy()
    s[1000:1005] ^= 1
    chk = err = 0
    for b in s:
        c, e = ck.bit(b)
        chk += c
        err += e
    assert ck.good == 0 and err == 5 and ck.state == bert_ref.IN_SYNC and chk == 2000 - 18


def _feed_frames(ck, start, n_frames, slip_after=None, erasure_rule=True):
    """clean BERT frames from PRBS index `start`; the frame at slip_after is lost (never reaches the checker)"""
    idx = start
    for f in range(n_frames):
        bits = _seq(idx, 197)
        idx = (idx + 197) % 511
        if f == slip_after:
            if erasure_rule:
                ck.erased()
            continue
        ck.frame(bits)


def test_literal_feed_after_a_lost_frame_stays_in_sync_at_half_ber():
    ck = bert_ref.Checker()
    _feed_frames(ck, 0, 60, slip_after=5, erasure_rule=False)
    before = list(ck.cnt)
    ck2 = bert_ref.Checker()
    _feed_frames(ck2, 0, 6)
    bits, errs = ck.cnt[0] - ck2.cnt[0], ck.cnt[1] - ck2.cnt[1]
    assert ck.state == bert_ref.IN_SYNC and before[5] == 0, "the literal checker never notices the slip"
    assert 0.45 < errs / bits < 0.55


def test_erasure_rule_keeps_ber_at_zero():
    ck = bert_ref.Checker()
    _feed_frames(ck, 0, 60, slip_after=5, erasure_rule=True)
    assert ck.state == bert_ref.IN_SYNC and ck.cnt[1] == 0 and ck.cnt[3] == 1 and ck.cnt[5] == 0
    assert ck.cnt[0] == 59 * 197 - 18


def test_bert_batch_through_the_oracle():
    import m17_sdr_amd as m
    C_, nblk, nf = 8, 40, 6
    sig = m.generate_bert_batch(C_, nblk, n_bert_frames=nf, ebn0_db=30.0)
    ref = oracle.Channels(C_).rx_blocks(sig["iq"], mode=1)
    for c in range(C_):
        r = ref["recs"][c, :ref["counts"][c]]
        aos = np.flatnonzero(r["flags"] & 0x100)
        assert len(aos) >= 3, f"channel {c}: {len(aos)} transmissions"
        # every complete transmission after the first (whose start the timing loop may miss while it settles from
        # reset): one AOS, then nf parsed BERT frames, then EOT
        for a, b in zip(aos[1:-1], aos[2:]):
            seg = r[a + 1:b]
            bert = seg[(seg["type"] == 4) & ((seg["flags"] & 0x2) != 0)]
            assert len(bert) == nf, f"channel {c}: {len(bert)} BERT frames in a transmission"
            assert ((seg["flags"] & 0x10) != 0).sum() == 1
    model = bert_ref.ChainModel(C_)
    model.call(ref)
    cnt = model.counters()
    # (not zero: the frame in front of the EOT shares a block with it, and the front end's per-block DC removal
    #  (m17_dsp.cpp:461-476) shifts its symbols by the EOT's mostly-+3 deviation -- the receiver's, not the checker's doing)
    assert cnt[:, 0].sum() > 0 and cnt[:, 1].sum() < 0.01 * cnt[:, 0].sum()
    assert cnt[:, 2].sum() == ((ref["recs"]["type"] == 4) & ((ref["recs"]["flags"] & 0x2) != 0)).sum()
