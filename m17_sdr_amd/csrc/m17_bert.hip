// m17_bert.hip -- the receive half of M17's BERT mode (included after m17_decode_quad.hip): the PRBS9 checker of
// m17_prbs9.cpp, fed with the decoded BERT frames of each channel in record order.
//
// The reference has the checker (m17_prbs9_rx_check, m17_prbs9.cpp:40-64) but never calls it: decode_bert_frame is
// empty (m17_rx_parse.cpp:178-180).  What reaches the checker is this library's definition (the "bert" option):
//   - a decoded BERT frame (type 4, parsed): its 197 bits, one m17_prbs9_rx_check each;
//   - an AOS record: m17_prbs9_rx_reset -- a transmission restarts its PRBS at index 0 (m17_tx_routines.cpp:224);
//   - any other parsed record while the checker is in sync: a BERT frame that was lost (its sync word was read as
//     another type).  The index moves on by the 197 bits the frame carried, none of them is checked.  Without this the
//     checker would never notice the slip: PRBS9 xor a shift of itself is another shift of PRBS9, which never has 18
//     ones in a row, so it would stay in sync and count half of all bits wrong from then on.
//
// The per-bit step is restated with its quirks: while hunting, the `eq_cnt >= 18` test comes before the reset on a
// mismatch, a mismatch resets the index to 0, m_rx_bad / m_rx_good are cleared on every bit; m_rx_good never counts
// (`d == 9`); sync drops only after 18 consecutive mismatches; m17_prbs9_rx_reset leaves eq_cnt and dif_cnt alone;
// all counters are uint16.
//
// One lane per channel (the records of a channel are a chain).  In sync, 32 bits go at a time: xor against the
// sequence's window at the index, popcount for the errors, and the 18-mismatch rule resolved over the word from the
// mismatch run carried in.  While hunting, one step per mismatch.
#pragma clang fp contract(off)

namespace m17dev {

constexpr int kPrbsLen = 511;                 // m17_prbs9.cpp:3
constexpr int kBertBits = 197;                // m17_tx_routines.cpp:228: PRBS bits per frame
constexpr int kPrbsWords = 18;                // the sequence, repeated, as 576 bits MSB first: any 32-bit window at 0..510

// The checker of one channel (m17_prbs9.cpp:6-12 for the first six fields) and its counters, 64 bytes.
struct BertChan {
    uint16_t idx, state, bad, good, eq, dif;   // m_rx_idx, m_rx_state, m_rx_bad, m_rx_good, m_rx_eq_cnt, m_rx_dif_cnt
    uint32_t pad;
    unsigned long long cnt[6];                 // bits checked in sync, errors among them, frames, erased frames, locks, losses
};
static_assert(sizeof(BertChan) == 64, "BertChan layout");
#define M17_BERT_NO_SYNC 0                      /* m17_prbs9.cpp:13-14 */
#define M17_BERT_IN_SYNC 1
#define M17_F_BERT_SYNC  0x0200u

// generate_prbs9 (m17_prbs9.cpp:16-27): x^9 + x^5 + 1 from 0x001, bit k of the sequence at bit 31 - (k & 31) of word k / 32
struct Prbs9Words { uint32_t w[kPrbsWords]; };
constexpr Prbs9Words make_prbs9_words()
{
    Prbs9Words P{};
    uint8_t seq[kPrbsLen] = {};
    uint32_t sr = 1;
    for (int i = 0; i < kPrbsLen; ++i) {
        const uint32_t bit = ((sr >> 8) ^ (sr >> 4)) & 1u;
        sr = ((sr << 1) | bit) & 0x1FFu;
        seq[i] = (uint8_t)bit;
    }
    for (int k = 0; k < 32 * kPrbsWords; ++k)
        if (seq[k % kPrbsLen]) P.w[k >> 5] |= 0x80000000u >> (k & 31);
    return P;
}
__constant__ Prbs9Words c_prbs9 = make_prbs9_words();
constexpr uint32_t kPrbsWord0 = make_prbs9_words().w[0];

struct BertRun {
    uint32_t checked = 0, errors = 0;
};

__device__ __forceinline__ uint32_t prbs_window(const uint32_t *P, uint32_t idx)            // bits idx .. idx + 31
{
    const unsigned long long v = ((unsigned long long)P[idx >> 5] << 32) | P[(idx >> 5) + 1];
    return (uint32_t)((v << (idx & 31u)) >> 32);
}
__device__ __forceinline__ uint32_t top_mask(uint32_t n) { return n >= 32 ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> n); }   // n >= 1

// n (1..32) received bits, MSB first in x, through the checker
__device__ __forceinline__ void bert_bits(BertChan &s, const uint32_t *P, uint32_t x, uint32_t n, BertRun &run)
{
    uint32_t pos = 0;
    while (pos < n) {
        if (s.state == M17_BERT_IN_SYNC) {
            // the rest of the word in sync: bit i of d (MSB first) = mismatch of bit pos + i
            const uint32_t m = n - pos;
            const uint32_t d = ((x << pos) ^ prbs_window(P, s.idx)) & top_mask(m);
            // mismatch runs of 18: bit b of z set <=> bits b .. b + 17 of v all set, v = d with the carried run
            // (s.dif < 18 in sync) above it; the first bit that completes a run is where sync drops
            const unsigned long long v = ((unsigned long long)((1u << s.dif) - 1u) << 32) | d;
            unsigned long long z = v & (v >> 1);
            z &= z >> 2; z &= z >> 4; z &= z >> 8; z &= z >> 2;
            const uint32_t zw = (uint32_t)z & top_mask(m);
            const uint32_t take = zw ? (uint32_t)__clz((int)zw) + 1u : m;           // bits handled in sync
            const uint32_t dt = d & top_mask(take);
            const uint32_t e = (uint32_t)__popc(dt);
            run.checked += take; run.errors += e;
            s.cnt[0] += take; s.cnt[1] += e;
            s.bad = (uint16_t)(s.bad + e);
            s.idx = (uint16_t)((s.idx + take) % kPrbsLen);
            if (zw) {
                s.dif = 18; s.eq = 0;                                               // the run that completes at 18
                s.state = M17_BERT_NO_SYNC; s.cnt[5]++;
            } else {
                const uint32_t t = dt >> (32u - take);                              // the word's bits, last one at bit 0
                if (t == 0) { s.eq = (uint16_t)(s.eq + take); s.dif = 0; }
                else if (!(t & 1u)) { s.eq = (uint16_t)__ffs((int)t) - 1; s.dif = 0; }
                else {
                    const uint32_t ones = (uint32_t)__ffs((int)~t) - 1u;            // trailing ones (t has a zero above them or is all ones)
                    s.dif = (uint16_t)((ones >= take) ? s.dif + take : ones);
                    s.eq = 0;
                }
            }
            pos += take;
        } else {
            // hunting: the bits up to the next mismatch match (eq_cnt counts up; the one that brings it to 18 locks), the
            // mismatch resets the index -- one pass per mismatch, not per bit
            // (after a mismatch the index is 0 and the window the sequence's first word, a constant: on bits that do not
            //  lock -- a false BERT sync -- this loop runs once per mismatch, and that is its whole chain)
            const uint32_t m = n - pos;
            const uint32_t win = s.idx ? prbs_window(P, s.idx) : kPrbsWord0;
            const uint32_t d = ((x << pos) ^ win) & top_mask(m);
            const uint32_t r = d ? (uint32_t)__clz((int)d) : m;                     // matching bits in front of it
            const uint32_t e1 = (uint32_t)(uint16_t)(s.eq + 1u);
            const uint32_t k = e1 >= 18u ? 0u : 18u - e1;                          // the matching bit that locks
            s.bad = 0; s.good = 0;
            if (k < r) {
                s.eq = (uint16_t)(s.eq + k + 1u); s.dif = 0;
                s.idx = (uint16_t)((s.idx + k + 1u) % kPrbsLen);
                s.state = M17_BERT_IN_SYNC; s.cnt[4]++;
                pos += k + 1u;
                continue;
            }
            if (r) { s.eq = (uint16_t)(s.eq + r); s.dif = 0; }
            pos += r;
            if (pos < n) {                                                          // the mismatch: m17_prbs9_rx_reset
                s.dif = (uint16_t)(s.dif + 1u); s.eq = 0;
                s.idx = 0;
                ++pos;
            } else {
                s.idx = (uint16_t)((s.idx + r) % kPrbsLen);
            }
        }
    }
}

// A frame that starts in sync and stays there -- no run of 18 mismatches, the one carried in included -- all at once:
// the seven words' windows, mismatches and run tests do not depend on each other (the start index fixes every window),
// so they are one short chain instead of seven dependent word steps.  Leaves s alone and returns false otherwise.
template <class Word>
__device__ __forceinline__ bool bert_frame_in_sync(BertChan &s, const uint32_t *P, Word word, BertRun &run)
{
    if (s.state != M17_BERT_IN_SYNC) return false;
    uint32_t d[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        uint32_t i = s.idx + 32u * k;
        if (i >= (uint32_t)kPrbsLen) i -= kPrbsLen;
        d[k] = word(k) ^ prbs_window(P, i);
    }
    d[6] &= top_mask(5);
    uint32_t runs = 0, e = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        // bit b of z (low half): bits b .. b + 17 of (previous word | this word) all mismatches; word 0 sees the carried run
        const uint32_t prev = k ? d[k - 1] : ((1u << s.dif) - 1u);
        const unsigned long long v = ((unsigned long long)prev << 32) | d[k];
        unsigned long long z = v & (v >> 1);
        z &= z >> 2; z &= z >> 4; z &= z >> 8; z &= z >> 2;
        runs |= (uint32_t)z;
        e += (uint32_t)__popc(d[k]);
    }
    if (runs) return false;
    run.checked = kBertBits; run.errors = e;
    s.cnt[0] += kBertBits; s.cnt[1] += e;
    s.bad = (uint16_t)(s.bad + e);
    s.idx = (uint16_t)((s.idx + kBertBits) % kPrbsLen);
    // the last 37 bits, last one at bit 0: the run of mismatches at the end (< 18 here) or of matches, which can be longer
    const unsigned long long T = ((unsigned long long)d[5] << 5) | (d[6] >> 27);
    if (T & 1ull) {
        s.dif = (uint16_t)__builtin_ctzll(~T); s.eq = 0;
    } else {
        s.dif = 0;
        if (T) s.eq = (uint16_t)__builtin_ctzll(T);
        else {
            uint32_t z = 37;
            int k = 4;
            while (k >= 0 && d[k] == 0) { z += 32; --k; }
            s.eq = (uint16_t)(k >= 0 ? z + (uint32_t)__ffs((int)d[k]) - 1u : s.eq + (uint32_t)kBertBits);
        }
    }
    return true;
}

// a decoded frame: 197 bits, MSB first, word(k) = bits 32 k .. 32 k + 31 (k = 6: 5 bits).  The word-by-word path (hunting,
// or a frame in which sync drops) is not unrolled: seven copies of its long step per call site made the kernel's code
// several times the instruction cache.
template <class Word>
__device__ __forceinline__ BertRun bert_frame(BertChan &s, const uint32_t *P, Word word)
{
    BertRun run;
    if (!bert_frame_in_sync(s, P, word, run)) {
#pragma unroll 1
        for (int k = 0; k < 7; ++k) bert_bits(s, P, word(k), k < 6 ? 32u : 5u, run);
    }
    s.cnt[2]++;
    return run;
}
__device__ __forceinline__ void bert_erased(BertChan &s)
{
    if (s.state == M17_BERT_IN_SYNC) { s.idx = (uint16_t)((s.idx + kBertBits) % kPrbsLen); s.cnt[3]++; }
}
__device__ __forceinline__ void bert_aos(BertChan &s) { s.idx = 0; s.state = M17_BERT_NO_SYNC; }     // m17_prbs9_rx_reset


// Sixteen channels per 64-lane workgroup.  The kernel is bound by the length of one channel's chain of records, not by
// memory: a counter pass over the earlier form (one lane per channel, each frame seven dependent word steps, four channels
// per wave) counted 13,300 VALU instructions per wave for ~12 frames a lane, 0.285 ms per call at 16,384 x 16
// (profiles/bert_pmc_checker.txt).  A frame in sync is now one short chain (bert_frame_in_sync), and the records come to
// LDS in batches of loads in flight together.
constexpr int BC_THREADS = 64;
constexpr int BC_CH = 16;                     // channels (lanes) per workgroup
constexpr int BC_RCH = 40;                    // records per channel staged in LDS at a time (30 KB)
constexpr int BC_BATCH = 10;                  // 16-byte loads per lane in flight at once
static_assert((BC_CH * BC_RCH * 3) % (BC_THREADS * BC_BATCH) == 0, "the staging loop's batches");
__device__ __forceinline__ int bert_away(const BertChan &s) { return (s.idx != 0 || s.state != M17_BERT_NO_SYNC) ? 1 : 0; }

// The full chain's checker, after the decoder and before the bookkeeping kernel (which zeroes nwork): one lane per
// channel, records in order.  nwork[3] = BERT frames of this call; *away_in != 0 when some checker ended the previous
// call away from its reset state (index 0, hunting) -- from there only a BERT frame changes a checker (an AOS resets to
// the same, an erasure needs sync), so with both zero the launch leaves at once.  *away_out (zeroed by k_worklist) is
// the same for this call; the host alternates the two words.
__global__ __launch_bounds__(BC_THREADS)
void k_bert_chain(m17gpu_rec_dev *__restrict__ recs, int rec_cap, const int32_t *__restrict__ counts, int C,
                  BertChan *__restrict__ st, const int32_t *__restrict__ nwork, const int32_t *__restrict__ away_in,
                  int32_t *__restrict__ away_out)
{
    if (nwork[3] == 0 && *away_in == 0) return;
    // the workgroup's BC_CH channels: words 0..11 of up to BC_RCH records each (type .. flags, data[0..28) at words 5..11)
    // come to LDS with all 64 lanes (a channel's records are contiguous), then lane k walks channel k's from there
    __shared__ uint32_t P[kPrbsWords];
    __shared__ uint4 L[BC_CH][BC_RCH][3];
    __shared__ int ncnt[BC_CH];
    const int c0 = (int)blockIdx.x * BC_CH, t = (int)threadIdx.x;
    if (t < kPrbsWords) P[t] = c_prbs9.w[t];
    if (t < BC_CH) ncnt[t] = (c0 + t < C) ? min(counts[c0 + t], rec_cap) : 0;
    __syncthreads();
    int nmax = 0;
#pragma unroll
    for (int k = 0; k < BC_CH; ++k) nmax = max(nmax, ncnt[k]);
    const int c = c0 + t;
    const bool mine = t < BC_CH && c < C;
    BertChan s;
    int n = 0;
    if (mine) { s = st[c]; n = ncnt[t]; }
    for (int base = 0; base < nmax; base += BC_RCH) {
#pragma unroll 1
        for (int b0 = 0; b0 < BC_CH * BC_RCH * 3; b0 += BC_THREADS * BC_BATCH) {
            uint4 v[BC_BATCH];
#pragma unroll
            for (int j = 0; j < BC_BATCH; ++j) {
                const int i = b0 + t + BC_THREADS * j, k = i / (BC_RCH * 3), rr = (i / 3) % BC_RCH, w = i % 3;
                v[j] = (base + rr < ncnt[k]) ? reinterpret_cast<const uint4 *>(recs + (size_t)(c0 + k) * rec_cap + base + rr)[w]
                                             : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int j = 0; j < BC_BATCH; ++j) {
                const int i = b0 + t + BC_THREADS * j, k = i / (BC_RCH * 3), rr = (i / 3) % BC_RCH, w = i % 3;
                L[k][rr][w] = v[j];
            }
        }
        __syncthreads();
        if (mine) {
            m17gpu_rec_dev *rc = recs + (size_t)c * rec_cap;
            const int rend = min(n - base, BC_RCH);
            for (int rr = 0; rr < rend; ++rr) {
                const uint4 w0 = L[t][rr][0], w2 = L[t][rr][2];
                const uint32_t type = w0.x & 0xFFu, flags = w0.y & 0xFFFFu;
                if (flags & M17_F_AOS) { bert_aos(s); continue; }
                if (!(flags & M17_F_PARSED)) continue;
                if (type != 4) { bert_erased(s); continue; }
                const uint32_t *lw = reinterpret_cast<const uint32_t *>(&L[t][rr][0]);
                const BertRun run = bert_frame(s, P, [&](int k) { return __builtin_bswap32(lw[5 + k]); });
                uint32_t *rw = reinterpret_cast<uint32_t *>(rc + base + rr);
                rw[11] = (w2.w & 0xFFu) | (run.checked << 8) | (run.errors << 16);          // data[24..27]
                if (s.state == M17_BERT_IN_SYNC) rw[1] = w0.y | M17_F_BERT_SYNC;
            }
        }
        __syncthreads();
    }
    if (mine) st[c] = s;
    if (__ballot(mine && bert_away(s)) != 0ull && t == 0) *away_out = 1;
}

// Stage entry: the same checker on a caller's streams.  bits [C][n][25] (197 bits, MSB first), kind [C][n]
// (0 decoded frame, 1 erased frame, 2 AOS), out [C][n][2] = bits checked in sync, errors.
__global__ __launch_bounds__(BC_THREADS)
void k_bert_feed(const uint8_t *__restrict__ bits, const uint8_t *__restrict__ kind, int n, int C,
                 BertChan *__restrict__ st, uint8_t *__restrict__ out, int32_t *__restrict__ away)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *away = 1;          // the word the next k_bert_chain reads: run it
    __shared__ uint32_t P[kPrbsWords];
    if (threadIdx.x < kPrbsWords) P[threadIdx.x] = c_prbs9.w[threadIdx.x];
    __syncthreads();
    const int c = (int)(blockIdx.x * BC_CH + threadIdx.x);
    if (threadIdx.x >= BC_CH || c >= C) return;
    BertChan s = st[c];
    for (int i = 0; i < n; ++i) {
        const size_t e = (size_t)c * n + i;
        const uint32_t k = kind[e];
        BertRun run;
        if (k == 2) bert_aos(s);
        else if (k == 1) bert_erased(s);
        else {
            const uint8_t *b = bits + e * 25;
            run = bert_frame(s, P, [&](int j) {
                uint32_t v = 0;
#pragma unroll
                for (int t = 0; t < 4; ++t) v = (v << 8) | ((4 * j + t < 25) ? (uint32_t)b[4 * j + t] : 0u);
                return v;
            });
        }
        out[2 * e] = (uint8_t)run.checked; out[2 * e + 1] = (uint8_t)run.errors;
    }
    st[c] = s;
}

} // namespace m17dev
