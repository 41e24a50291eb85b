// lpc_flat_check.cpp — host check of the FMA range K1's autocorrelation uses
// (python-audio-tools_amd/csrc/lpc_flat.h) against the Tukey(0.5) table the
// engine builds (tukey() in engine.hip, repeated here expression for
// expression), and of the exactness argument itself.
//
// (a) For every N in [14, 4608] and 8192, 16384, 65535, and the margins of the
//     three K1 instantiations (8, 12, 32): every table entry in the header's
//     range, and the `lags` entries before its start, is exactly 1.0.
// (b) Block lengths 4096 4608 576 256 208 192 160 57 (for 52-sample groups at
//     lags 12: no flat group at 192 and 57, exactly one at 256, a first group
//     starting at the range's start at 576 and 160, a last group ending at its
//     end at 208 -- asserted), stereo 16-bit with the four candidates left,
//     right, mid, side, five signal kinds: the 13 sums with std::fma inside the
//     range and multiply-then-add outside equal multiply-then-add everywhere,
//     bit for bit.  Three granularities: per sample, the kernel's 52-sample
//     groups followed by 13-sample groups, and 13-sample groups alone.
// (c) The same with the range widened by one sample at its start, and at its
//     end: noise input has to show mismatches, or (b) proves nothing.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -o lpc_flat_check tools/lpc_flat_check.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../python-audio-tools_amd/csrc/lpc_flat.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

static void tukey(uint32_t N, double *w)
{
    const double alpha = 0.5;
    const unsigned window1 = (unsigned)(alpha * (N - 1)) / 2;
    const unsigned window2 = (unsigned)((N - 1) * (1.0 - (alpha / 2.0)));
    for (unsigned n = 0; n < N; n++) {
        if (n <= window1)
            w[n] = 0.5 * (1.0 + std::cos(M_PI * (((2 * n) / (alpha * (N - 1))) - 1.0)));
        else if (n <= window2)
            w[n] = 1.0;
        else
            w[n] = 0.5 * (1.0 + std::cos(M_PI * (((2.0 * n) / (alpha * (N - 1))) -
                                                 (2.0 / alpha) + 1.0)));
    }
}

static const int LAGS = 12, K = LAGS + 1;

static uint32_t g_rng = 2463534242u;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 17;
    g_rng ^= g_rng << 5;
    return g_rng;
}

enum { SIG_NOISE, SIG_SIDE_FULL, SIG_SINE, SIG_SILENCE, SIG_LOUD_FLAT, SIG_KINDS };

static void make_signal(int kind, uint32_t N, int trial, std::vector<int16_t> &l,
                        std::vector<int16_t> &r)
{
    l.assign(N, 0);
    r.assign(N, 0);
    const LpcFlatRange fr = lpc_flat_range(N, 0);
    for (uint32_t n = 0; n < N; ++n) {
        switch (kind) {
        case SIG_NOISE: // side = l - r covers the full 17-bit range
            l[n] = (int16_t)(rnd() >> 16);
            r[n] = (int16_t)(rnd() >> 16);
            break;
        case SIG_SIDE_FULL: // |side| = 65535, sign alternating
            l[n] = (n + trial) & 1 ? -32768 : 32767;
            r[n] = (n + trial) & 1 ? 32767 : -32768;
            break;
        case SIG_SINE: {
            const double a = 30000.0 * std::sin(0.01 * (trial + 1) * n);
            l[n] = (int16_t)(a + (int)(rnd() % 2001) - 1000);
            r[n] = (int16_t)(0.5 * a + (int)(rnd() % 201) - 100);
            break;
        }
        case SIG_SILENCE:
            break;
        case SIG_LOUD_FLAT: // loud only where the window is the literal 1.0
            if (n >= fr.lo && n < fr.hi) {
                l[n] = (int16_t)(rnd() >> 16);
                r[n] = (int16_t)(rnd() >> 16);
            }
            break;
        }
    }
}

static int32_t candidate(int c, int32_t l, int32_t r)
{
    return c == 0 ? l : c == 1 ? r : c == 2 ? (l + r) >> 1 : l - r;
}

// use_fma[n]: sample n updates its 13 accumulators with std::fma and takes
// x = (double)s; otherwise x = (double)s * w, rounded multiply, rounded add
static void sums(const std::vector<int32_t> &s, const std::vector<double> &w,
                 const std::vector<uint8_t> &use_fma, double (&acc)[K])
{
    double hist[K];
    for (int k = 0; k < K; ++k)
        acc[k] = hist[k] = 0.0;
    const uint32_t N = (uint32_t)s.size();
    for (uint32_t n = 0; n < N; ++n) {
        const int u = (int)(n % K);
        const bool f = use_fma[n] != 0;
        const double x = f ? (double)s[n] : (double)s[n] * w[n];
        hist[u] = x;
        for (int L = 0; L < K; ++L) {
            const double h = hist[(u - L + K) % K];
            if (f) {
                acc[L] = std::fma(h, x, acc[L]);
            } else {
                const double prod = h * x;
                acc[L] = acc[L] + prod;
            }
        }
    }
}

static void mark(std::vector<uint8_t> &m, const LpcFlatRange &fr, uint32_t from, uint32_t to,
                 uint32_t group)
{
    for (uint32_t j = from; j + group <= to; j += group)
        if (lpc_flat_group(fr, j, group))
            for (uint32_t n = j; n < j + group; ++n)
                m[n] = 1;
}

static uint64_t differ(const double (&a)[K], const double (&b)[K])
{
    uint64_t d = 0;
    for (int k = 0; k < K; ++k)
        d += std::memcmp(&a[k], &b[k], sizeof(double)) != 0;
    return d;
}

int main()
{
    uint64_t cases = 0, bad = 0;
    // (a)
    std::vector<uint32_t> all_n;
    for (uint32_t N = 14; N <= 4608; ++N)
        all_n.push_back(N);
    for (uint32_t N : {8192u, 16384u, 65535u})
        all_n.push_back(N);
    std::vector<double> w;
    for (uint32_t N : all_n) {
        w.resize(N);
        tukey(N, w.data());
        for (uint32_t lags : {8u, 12u, 32u}) {
            const LpcFlatRange fr = lpc_flat_range(N, lags);
            ++cases;
            bool ok = fr.lo <= fr.hi && fr.hi <= N && (fr.lo == fr.hi || fr.lo >= lags);
            if (ok && fr.lo < fr.hi)
                for (uint32_t n = fr.lo - lags; n < fr.hi; ++n)
                    ok = ok && w[n] == 1.0;
            if (!ok) {
                if (bad < 8)
                    printf("range N %u lags %u: [%u, %u) not flat\n", N, lags, fr.lo, fr.hi);
                ++bad;
            }
        }
    }
    // the group properties (b) relies on, 52-sample groups at lags 12
    {
        struct { uint32_t N; int groups; bool at_lo, at_hi; } want[] = {
            {192, 0, false, false}, {57, 0, false, false}, {256, 1, false, false},
            {576, -1, true, false}, {160, -1, true, false}, {208, -1, false, true}};
        for (auto &q : want) {
            const LpcFlatRange fr = lpc_flat_range(q.N, LAGS);
            int groups = 0;
            bool at_lo = false, at_hi = false;
            for (uint32_t j = 0; j + 52 <= q.N; j += 52)
                if (lpc_flat_group(fr, j, 52)) {
                    ++groups;
                    at_lo = at_lo || j == fr.lo;
                    at_hi = at_hi || j + 52 == fr.hi;
                }
            ++cases;
            if ((q.groups >= 0 && groups != q.groups) || (q.groups < 0 && groups < 1) ||
                (q.at_lo && !at_lo) || (q.at_hi && !at_hi)) {
                printf("groups N %u: %d groups, at_lo %d at_hi %d\n", q.N, groups, at_lo, at_hi);
                ++bad;
            }
        }
    }
    // (b) and (c)
    uint64_t wide_lo = 0, wide_hi = 0;
    std::vector<int16_t> l, r;
    for (uint32_t N : {4096u, 4608u, 576u, 256u, 208u, 192u, 160u, 57u}) {
        w.resize(N);
        tukey(N, w.data());
        const LpcFlatRange fr = lpc_flat_range(N, LAGS);
        std::vector<uint8_t> none(N, 0), per_sample(N, 0), g52(N, 0), g13(N, 0), wlo(N, 0),
            whi(N, 0);
        for (uint32_t n = fr.lo; n < fr.hi; ++n)
            per_sample[n] = wlo[n] = whi[n] = 1;
        mark(g52, fr, 0, N / 52 * 52, 52);
        mark(g52, fr, N / 52 * 52, N / 13 * 13, 13);
        mark(g13, fr, 0, N / 13 * 13, 13);
        if (fr.lo < fr.hi) {
            wlo[fr.lo - 1] = 1;
            whi[fr.hi] = 1; // hi <= N - 1: the last sample is never flat
        }
        for (int kind = 0; kind < SIG_KINDS; ++kind)
            for (int trial = 0; trial < 12; ++trial) {
                make_signal(kind, N, trial, l, r);
                for (int c = 0; c < 4; ++c) {
                    std::vector<int32_t> s(N);
                    for (uint32_t n = 0; n < N; ++n)
                        s[n] = candidate(c, l[n], r[n]);
                    double ref[K], got[K];
                    sums(s, w, none, ref);
                    for (const std::vector<uint8_t> *m : {&per_sample, &g52, &g13}) {
                        sums(s, w, *m, got);
                        ++cases;
                        if (differ(ref, got)) {
                            if (bad < 24)
                                printf("sums N %u kind %d trial %d cand %d differ\n", N, kind,
                                       trial, c);
                            ++bad;
                        }
                    }
                    if (kind == SIG_NOISE && fr.lo < fr.hi) {
                        sums(s, w, wlo, got);
                        wide_lo += differ(ref, got) != 0;
                        sums(s, w, whi, got);
                        wide_hi += differ(ref, got) != 0;
                    }
                }
            }
    }
    printf("cases %llu bad %llu wide_lo %llu wide_hi %llu\n", (unsigned long long)cases,
           (unsigned long long)bad, (unsigned long long)wide_lo, (unsigned long long)wide_hi);
    return (bad || !wide_lo || !wide_hi) ? 1 : 0;
}
