// False reads of a locus from its chromosome: where the keyword prefilter would wrongly let a read through
// (VNTRFinder.simulate_false_filtered_reads, vntr_finder.py:927-973; vntr_extras.simulate_false_filtered_reads is the
// numpy mirror this restates).  For one chromosome of n bytes and one locus with VNTR [vs, ve):
//   keyword    an 11-mer of get_keywords_for_filtering(..., True, 11) made of A/C/G/T only (case-insensitive)
//   examined   position i with 1 <= i < n - 11 whose bases [i-1, i+11) are all A/C/G/T, case-insensitively
//   hit        an examined i whose 11-mer is a keyword and not vs - 150 < i < ve
//   triple     after each hit p: when the locus has >= 3 hits and p[-1] - p[-3] < 150, reads start at
//              j in range(p[-1] - 150, p[-3], 5); the read is s[j:j+150] as a Python slice (j may be negative) and is
//              kept when it holds no N / n (other IUPAC codes pass)
//   cap        after a hit's reads are added, a locus holding more than 10 000 reads stops (so at most 10 030)
// The window, the position test, the slice and the per-locus fold are host + device code; the host twin walks every
// position with them, the scan kernel finds the hits and the host folds them in chromosome order.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GSCAN_HD __host__ __device__
#else
#define GSCAN_HD
#endif

namespace gscan {

const int K = 11;                                   // keyword size
const int READ = 150;                               // read size
const int STEP = 5;                                 // read start step
const int MIN_MATCH = 3;
const int32_t MAX_READS = 10000;
const int32_t READ_CAPACITY = MAX_READS + READ / STEP;   // reads one locus can hold when it stops
const uint32_t KMER_MASK = (1u << (2 * K)) - 1;
const int64_t N_KMERS = (int64_t)1 << (2 * K);

GSCAN_HD inline uint32_t base_code(uint8_t c)       // A/C/G/T in either case -> 0..3, anything else 4
{
    switch (c | 0x20) {
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 't': return 3;
    default: return 4;
    }
}

GSCAN_HD inline bool is_n(uint8_t c) { return c == 'N' || c == 'n'; }

// the last K + 1 bases pushed: value of the last K, length of the clean run ending at the last one (capped at K + 1)
struct Window {
    uint32_t value;
    int32_t run;
};

GSCAN_HD inline void window_init(Window &w) { w.value = 0; w.run = 0; }

GSCAN_HD inline void window_push(Window &w, uint8_t c)
{
    const uint32_t code = base_code(c);
    if (code > 3) { w.run = 0; return; }
    w.value = ((w.value << 2) | code) & KMER_MASK;
    w.run = w.run < K + 1 ? w.run + 1 : K + 1;
}

// after pushing base q: position i = q - K + 1 has bases [i-1, i+K) all clean
GSCAN_HD inline bool window_ready(const Window &w) { return w.run >= K + 1; }

GSCAN_HD inline bool position_in_range(int64_t i, int64_t n) { return i >= 1 && i < n - K; }

GSCAN_HD inline bool excluded(int64_t i, int64_t vs, int64_t ve) { return vs - READ < i && i < ve; }

GSCAN_HD inline int64_t slice_index(int64_t x, int64_t n) { return x < 0 ? (x + n < 0 ? 0 : x + n) : (x > n ? n : x); }

// s[j:j+READ] of a Python str of length n -> [a, b)
GSCAN_HD inline void read_slice(int64_t j, int64_t n, int64_t *a, int64_t *b)
{
    const int64_t s = slice_index(j, n), e = slice_index(j + READ, n);
    *a = s;
    *b = e < s ? s : e;
}

GSCAN_HD inline bool holds_n(const uint8_t *s, int64_t a, int64_t b)
{
    for (int64_t k = a; k < b; ++k)
        if (is_n(s[k])) return true;
    return false;
}

struct LocusState {
    int64_t p[MIN_MATCH];          // the last MIN_MATCH hits, oldest first
    int64_t hits;
    int32_t reads;
    int32_t live;
};

GSCAN_HD inline void locus_init(LocusState &st)
{
    for (int k = 0; k < MIN_MATCH; ++k) st.p[k] = 0;
    st.hits = 0;
    st.reads = 0;
    st.live = 1;
}

// fold a keyword hit at i into a live locus; reads go to rb / re[st.reads...] (capacity READ_CAPACITY)
GSCAN_HD inline void locus_hit(LocusState &st, int64_t i, const uint8_t *s, int64_t n, int64_t vs, int64_t ve, int64_t *rb,
                               int64_t *re)
{
    if (excluded(i, vs, ve)) return;
    for (int k = 0; k + 1 < MIN_MATCH; ++k) st.p[k] = st.p[k + 1];
    st.p[MIN_MATCH - 1] = i;
    ++st.hits;
    if (st.hits >= MIN_MATCH && st.p[MIN_MATCH - 1] - st.p[0] < READ)
        for (int64_t j = st.p[MIN_MATCH - 1] - READ; j < st.p[0]; j += STEP) {
            int64_t a, b;
            read_slice(j, n, &a, &b);
            if (holds_n(s, a, b)) continue;
            rb[st.reads] = a;
            re[st.reads] = b;
            ++st.reads;
        }
    if (st.reads > MAX_READS) st.live = 0;
}

}  // namespace gscan
