"""Expected values of BERT receive (the "bert" option): frame decode through the oracle's exported primitives, and a
Python restatement of the reference's PRBS9 checker with this library's feed rules.  TEST INFRASTRUCTURE ONLY.

Decode (the inverse of m17_fmt_add_bert_frame, m17_tx_routines.cpp:226-238; decode_bert_frame itself is empty,
m17_rx_parse.cpp:178-180): demap, de-randomise and de-interleave the 368 soft bits as the other frame types do
(oracle/m17_oracle.c:746-750), append one erasure for the coded bit the transmitter never sends, P2 de-puncture to 402,
Viterbi over 201 steps, keep bits[1..197] (the offset of oracle/m17_oracle.c:751-753, 787-789).

Checker: m17_prbs9_rx_check / m17_prbs9_rx_reset (m17_prbs9.cpp:36-64), quirks kept.  Feed, per channel in record
order: a decoded BERT frame -> its 197 bits; an AOS record -> m17_prbs9_rx_reset; any other parsed record while in
sync -> the index moves on by 197 (an erased BERT frame)."""
import ctypes as C

import numpy as np

from tests import oracle

PRBS_LEN = 511          # m17_prbs9.cpp:3
BERT_BITS = 197         # m17_tx_routines.cpp:228
NO_SYNC, IN_SYNC = 0, 1  # m17_prbs9.cpp:13-14
F_BERT_SYNC = 0x200


def prbs9(n=PRBS_LEN):
    out = np.zeros(n, np.uint8)
    oracle.L().m17o_prbs9(oracle.vp(out), n)
    return out


PRBS = prbs9()


def bert_frame_dibits(idx):
    """(dibits[192], next idx) built from the oracle's transmit primitives: m17_fmt_add_bert_frame."""
    L = oracle.L()
    bits = np.zeros(201, np.uint8)
    bits[:197] = PRBS[(idx + np.arange(197)) % PRBS_LEN]
    coded = np.zeros(402, np.uint8)
    L.m17o_conv_encode_1(oracle.vp(bits), oracle.vp(coded), 197)       # 197 bits + the 4-step zero tail = 402
    punc = np.zeros(402, np.uint8)
    n = L.m17o_punc(2, oracle.vp(coded), oracle.vp(punc), 402)
    assert n == 369
    il = np.zeros(368, np.uint8)
    L.m17o_interleave_u8(oracle.vp(np.ascontiguousarray(punc[:368])), oracle.vp(il), 368)
    rnd = np.zeros(368, np.uint8)
    L.m17o_de_correlate_u8(oracle.vp(il), oracle.vp(rnd), 368)
    d = np.zeros(192, np.uint8)
    for i in range(8):
        d[i] = (0xDF55 >> (14 - 2 * i)) & 3
    d[8:] = (rnd[0::2] << 1) | rnd[1::2]
    return d, (idx + 197) % PRBS_LEN


def decode_frame(sym):
    """float32 symbols [192] -> 197 bits packed MSB first into 25 bytes."""
    L = oracle.L()
    sym = np.ascontiguousarray(sym, np.float32)
    sb = np.zeros(384, np.float32)
    L.m17o_demap_frame(oracle.vp(sym), oracle.vp(sb))
    L.m17o_de_correlate_f(oracle.vp(sb), oracle.vp(sb), 368)
    so0 = np.zeros(369, np.float32)                                    # so0[368] = 0.0f: the erasure
    L.m17o_de_interleave(oracle.vp(sb), oracle.vp(so0), 368)
    so1 = np.zeros(402, np.float32)
    L.m17o_de_punc(2, oracle.vp(so0), oracle.vp(so1), 402)
    bits = np.zeros(201, np.uint8)
    L.m17o_viterbi_decode(oracle.vp(so1), oracle.vp(bits), 402)
    return np.packbits(bits[1:198])


def unpack(b25):
    return np.unpackbits(np.asarray(b25, np.uint8))[:BERT_BITS]


class Checker:
    """m17_prbs9.cpp:6-12 statics of one receiver, all 0 at start, plus the library's counters."""

    def __init__(self):
        self.idx = self.state = self.bad = self.good = self.eq = self.dif = 0
        self.cnt = [0] * 6      # bits checked in sync, errors, frames, erased, locks, losses

    def reset(self):            # m17_prbs9_rx_reset, m17_prbs9.cpp:36-39: idx and state only
        self.idx = 0
        self.state = NO_SYNC

    def bit(self, b):
        """m17_prbs9_rx_check, m17_prbs9.cpp:40-64.  Returns (checked in sync, error)."""
        d = int(b) ^ int(PRBS[self.idx])
        if d:
            self.dif = (self.dif + 1) & 0xFFFF
            self.eq = 0
        else:
            self.eq = (self.eq + 1) & 0xFFFF
            self.dif = 0
        self.idx = (self.idx + 1) % PRBS_LEN
        if self.state == NO_SYNC:
            self.bad = 0
            self.good = 0
            if self.eq >= 18:                    # :54, before the reset of :55
                self.state = IN_SYNC
                self.cnt[4] += 1
            if d:
                self.reset()
            return 0, 0
        if self.dif >= 18:                       # :57
            self.state = NO_SYNC
            self.cnt[5] += 1
        if d:
            self.bad = (self.bad + 1) & 0xFFFF
        if d == 9:                               # :59, never
            self.good = (self.good + 1) & 0xFFFF
        self.cnt[0] += 1
        self.cnt[1] += d
        return 1, d

    def frame(self, bits197):
        chk = err = 0
        for b in bits197:
            c, e = self.bit(b)
            chk += c
            err += e
        self.cnt[2] += 1
        return chk, err

    def erased(self):
        if self.state == IN_SYNC:
            self.idx = (self.idx + BERT_BITS) % PRBS_LEN
            self.cnt[3] += 1

    def aos(self):
        self.reset()

    def state_row(self):
        return [self.idx, self.state, self.bad, self.good, self.eq, self.dif]


class ChainModel:
    """The BERT fields of the full chain's records, from the oracle's records and recovered symbols, call by call."""

    def __init__(self, n_channels):
        self.C = n_channels
        self.chk = [Checker() for _ in range(n_channels)]
        self.tail = [np.zeros(0, np.float32) for _ in range(n_channels)]   # symbols of earlier calls (the last 191)
        self.block0 = 0

    def call(self, ref, channels=None):
        """ref = oracle.Channels.rx_blocks(...) of one call.  Returns recs with the BERT fields patched in (a copy) for
        the given channels (default all); the others' rows are left as the oracle's."""
        recs = ref["recs"].copy()
        nblk = ref["nsyms"].shape[1]
        chans = range(self.C) if channels is None else channels
        for c in chans:
            ns = ref["nsyms"][c]
            stream = np.concatenate([self.tail[c], ref["syms"][c, :int(ns.sum())]])
            base = len(self.tail[c])
            starts = base + np.concatenate([[0], np.cumsum(ns)[:-1]])
            ck = self.chk[c]
            n = min(int(ref["counts"][c]), recs.shape[1])
            for r in range(n):
                rec = recs[c, r]
                fl = int(rec["flags"])
                if fl & oracle_flag("AOS"):
                    ck.aos()
                    continue
                if not fl & oracle_flag("PARSED"):
                    continue
                if rec["type"] != 4:
                    ck.erased()
                    continue
                end = int(starts[int(rec["block"]) - self.block0]) + int(rec["sym_pos"])
                sym = stream[end - 191:end + 1]
                assert len(sym) == 192
                data = decode_frame(sym)
                chk, err = ck.frame(unpack(data))
                rec["data"][:25] = data
                rec["data"][25] = chk
                rec["data"][26] = err
                if ck.state == IN_SYNC:
                    rec["flags"] = fl | F_BERT_SYNC
            self.tail[c] = stream[-191:].copy()
        self.block0 += nblk
        return recs

    def counters(self):
        return np.array([ck.cnt for ck in self.chk], np.uint64)

    def states(self):
        return np.array([ck.state_row() for ck in self.chk], np.int32)


def oracle_flag(name):
    return {"PARSED": 0x2, "AOS": 0x100}[name]
