// bits_crc_check.cpp — host check of the device-side commons that compile for
// the host: the LSB-first bit reader (python-audio-tools_amd/csrc/bits_lsb.h)
// and the CRC table builders and advance (csrc/crc_common.h).  No GPU, no HIP.
//
// Reader: both word fetches (LsbReader<false>, LsbReader<true>) against a
// reader that takes one bit at a time.  Every buffer is a heap block of exactly its length (rounded up to 4 for
// LsbReader<false>, as the TTA batch buffer is), so under AddressSanitizer
// a read outside it stops the program; the bytes around the range are the
// complement of what a leak would have to look like to go unnoticed (random,
// so a reader that lets them in disagrees with the reference).
//   ranges   every start offset mod 4, lengths 0-9 bytes, ending 0-3 bytes
//            before the buffer's end; before the call under test 0 .. all of
//            the range's bits are consumed, so that unary() and bits(n),
//            n = 0, 1, 31, 32, run at every fill level of the accumulator
//            (all of 0..64 are asserted to have been met) and at the range's
//            end; the rest of the range is then drained a bit at a time.
//   runs     unary runs of 0, 31, 32, 33, 63, 64 and 65 ones at bit phases
//            0-39, ended by a 0 bit and ended by the range (false).
//
// CRC: CRC-16 0x8005 and CRC-32 0x04C11DB7 (MSB first, init 0).
//   the byte table and slicing by 4 against a bitwise CRC on random strings
//     of 0-70 bytes;
//   advance(crc(A), |B|) ^ crc(B) == crc(A || B) for |B| up to 2^17;
//   the tables byte for byte against the builders this header replaced
//     (engine.hip, flac_decode.hip, ogg_demux.hip), kept below as they were.
//
// Build and run:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined
//       -fno-sanitize-recover=all -o bits_crc_check tools/bits_crc_check.cpp
//   ./bits_crc_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../python-audio-tools_amd/csrc/bits_lsb.h"
#include "../python-audio-tools_amd/csrc/crc_common.h"

static uint64_t g_cases = 0, g_bad = 0;
static uint32_t g_rng = 2463534242u;

static uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 17;
    g_rng ^= g_rng << 5;
    return g_rng;
}

static void fail(const char *what, long a, long b, long c, long d)
{
    if (g_bad++ < 20)
        fprintf(stderr, "FAIL %s (%ld %ld %ld %ld)\n", what, a, b, c, d);
}

// ------------------------------------------------------------------ reader
// the reference: bit i of the range is bit i % 8 of its byte i / 8
struct RefBits {
    const uint8_t *p;
    uint64_t at, n; // next bit, bits in the range
    bool bit() { const bool b = (p[at >> 3] >> (at & 7)) & 1; ++at; return b; }
    bool unary(uint32_t &count)
    {
        count = 0;
        while (at < n) {
            if (!bit())
                return true;
            ++count;
        }
        return false; // the range is used up
    }
    bool bits(uint32_t k, uint32_t &v)
    {
        if (n - at < k)
            return false; // nothing taken
        uint64_t x = 0;
        for (uint32_t i = 0; i < k; ++i)
            x |= (uint64_t)bit() << i;
        v = (uint32_t)x;
        return true;
    }
};

// a heap block of exactly `len` bytes holding random bytes, the range's own
// bytes [s, s + L) from `fill` where given
static uint8_t *make_buf(size_t len, size_t s, size_t L, const uint8_t *fill)
{
    uint8_t *b = (uint8_t *)malloc(len ? len : 1);
    if (!b)
        abort();
    for (size_t i = 0; i < len; ++i)
        b[i] = (uint8_t)rnd();
    if (fill && L)
        memcpy(b + s, fill, L);
    return b;
}

// the buffer a reader is given: LsbReader<false> loads whole words, so its
// buffer's length is a multiple of 4; LsbReader<true> is told the length
template <bool LIMITED> static size_t buf_length(size_t len)
{
    return LIMITED ? len : (len + 3) & ~(size_t)3;
}
template <bool LIMITED>
static LsbReader<LIMITED> open_reader(const uint8_t *b, size_t len, size_t s, size_t L)
{
    LsbReader<LIMITED> r;
    r.data = b;
    r.pos = s;
    r.end = s + L;
    r.limit = LIMITED ? len : 0; // unused by LsbReader<false>
    return r;
}

static bool g_level[5][65]; // fill levels met on entry: unary, bits 0, 1, 31, 32
static const uint32_t kWidths[4] = {0, 1, 31, 32};

// one call of both readers (op 0: unary, 1-4: bits(kWidths[op - 1])), compared
template <typename R> static bool step(R &r, RefBits &ref, int op, long tag)
{
    uint32_t a = 0, b = 0;
    bool oa, ob;
    g_level[op][r.have] = true;
    if (op == 0) {
        oa = r.unary(a);
        ob = ref.unary(b);
    } else {
        oa = r.bits(kWidths[op - 1], a);
        ob = ref.bits(kWidths[op - 1], b);
    }
    ++g_cases;
    // what a failed unary() counted is not used by the decoders
    if (oa != ob || (oa && a != b)) {
        fail("reader", tag, op, (long)a, (long)b);
        return false;
    }
    return true;
}

template <bool LIMITED> static void check_ranges()
{
    for (size_t s = 0; s < 4; ++s)
        for (size_t L = 0; L <= 9; ++L)
            for (size_t gap = 0; gap < 4; ++gap)
                for (int op = 0; op < 5; ++op)
                    for (size_t pre = 0; pre <= 8 * L; ++pre) {
                        const size_t len = buf_length<LIMITED>(s + L + gap);
                        // a quarter of the ranges all ones: runs reach the end
                        std::vector<uint8_t> ones(L, 0xFF);
                        uint8_t *b = make_buf(len, s, L, (pre + L) % 4 == 0 ? ones.data() : nullptr);
                        LsbReader<LIMITED> r = open_reader<LIMITED>(b, len, s, L);
                        RefBits ref = {b + s, 0, 8 * L};
                        const long tag = (long)(s * 1000000 + L * 10000 + gap * 1000 + pre);
                        bool ok = step(r, ref, 1, tag); // bits(0): a refill alone
                        for (size_t left = pre; ok && left;) { // take `pre` bits
                            const uint32_t k = left >= 32 ? 32u : (left >= 31 ? 31u : 1u);
                            ok = step(r, ref, k == 32 ? 4 : (k == 31 ? 3 : 2), tag);
                            left -= k;
                        }
                        ok = ok && step(r, ref, op, tag);
                        for (size_t i = 0; ok && i <= 8 * L; ++i) // drain, and once past the end
                            ok = step(r, ref, 2, tag);
                        if (ok && (ref.at != ref.n || r.have != 0 || r.pos != r.end))
                            fail("drain", tag, op, (long)r.have, (long)(r.end - r.pos));
                        free(b);
                    }
}

template <bool LIMITED> static void check_runs()
{
    static const uint32_t kRuns[7] = {0, 31, 32, 33, 63, 64, 65};
    for (size_t s = 0; s < 4; ++s)
        for (size_t gap = 0; gap < 4; ++gap)
            for (uint32_t ph = 0; ph < 40; ++ph)
                for (uint32_t run : kRuns)
                    for (int ended = 0; ended < 2; ++ended) {
                        // ph random bits, `run` ones, then a 0 bit and random bits
                        // (ended) or ones up to the range's end
                        const size_t bitsn = ph + run + (ended ? 1 + rnd() % 40 : 0);
                        const size_t L = (bitsn + 7) / 8;
                        std::vector<uint8_t> img(L);
                        for (size_t i = 0; i < 8 * L; ++i) {
                            bool v = rnd() & 1;
                            if (i >= ph)
                                v = i < ph + run || (!ended) || (i > ph + run && v);
                            img[i >> 3] = (uint8_t)(img[i >> 3] | (v << (i & 7)));
                        }
                        const size_t len = buf_length<LIMITED>(s + L + gap);
                        uint8_t *b = make_buf(len, s, L, img.data());
                        LsbReader<LIMITED> r = open_reader<LIMITED>(b, len, s, L);
                        RefBits ref = {b + s, 0, 8 * L};
                        const long tag = (long)(s * 1000000 + gap * 100000 + ph * 1000 + run);
                        bool ok = true;
                        for (uint32_t left = ph; ok && left;) {
                            const uint32_t k = left >= 32 ? 32u : (left >= 31 ? 31u : 1u);
                            ok = step(r, ref, k == 32 ? 4 : (k == 31 ? 3 : 2), tag);
                            left -= k;
                        }
                        if (ok) {
                            uint32_t got = 0;
                            const bool res = r.unary(got);
                            ++g_cases;
                            if (res != (ended != 0) || (ended && got != run))
                                fail("run", tag, ended, (long)got, (long)res);
                            if (!ended && (r.have != 0 || r.pos != r.end))
                                fail("run end", tag, ended, (long)r.have, 0);
                        }
                        free(b);
                    }
}

// --------------------------------------------------------------------- CRC
template <int W> static uint32_t crc_bitwise(uint32_t poly, const uint8_t *p, size_t n, uint32_t c)
{
    const uint32_t top = 1u << (W - 1), mask = (top - 1u) | top;
    for (size_t i = 0; i < n; ++i) {
        c ^= (uint32_t)p[i] << (W - 8);
        for (int k = 0; k < 8; ++k)
            c = (c & top) ? (c << 1) ^ poly : c << 1;
        c &= mask;
    }
    return c;
}

// the kernels' loops: big-endian words through the four slicing tables, the
// tail through the byte table
template <int W> static uint32_t crc_sliced(const uint32_t *t, const uint8_t *p, size_t n)
{
    const uint32_t top = 1u << (W - 1), mask = (top - 1u) | top;
    uint32_t c = 0;
    size_t i = 0;
    for (; i + 4 <= n; i += 4) {
        const uint32_t w = ((uint32_t)p[i] << 24) | ((uint32_t)p[i + 1] << 16) |
                           ((uint32_t)p[i + 2] << 8) | p[i + 3];
        const uint32_t x = w ^ (W == 32 ? c : c << (32 - W));
        c = t[3 * 256 + (x >> 24)] ^ t[2 * 256 + ((x >> 16) & 0xFFu)] ^
            t[256 + ((x >> 8) & 0xFFu)] ^ t[x & 0xFFu];
    }
    for (; i < n; ++i)
        c = ((c << 8) ^ t[((c >> (W - 8)) ^ p[i]) & 0xFFu]) & mask;
    return c;
}

template <int W> static uint32_t advance(const uint32_t *adv, uint32_t c, uint64_t bytes)
{
    for (int m = 0; bytes; ++m, bytes >>= 1)
        if (bytes & 1u)
            c = crc_advance<W>(adv + m * W, c);
    return c;
}

template <int W> static void check_crc(uint32_t poly)
{
    constexpr int M = 18; // up to 2^18 - 1 bytes
    static uint32_t t[4 * 256], adv[M * W];
    crc_build_tables<W>(poly, t, 4);
    crc_build_advance<W>(t, adv, M);
    std::vector<uint8_t> buf(70 + (1u << 17));
    for (uint8_t &x : buf)
        x = (uint8_t)rnd();
    for (int rep = 0; rep < 40; ++rep)
        for (size_t n = 0; n <= 70; ++n) {
            const uint8_t *p = buf.data() + rnd() % (buf.size() - 70);
            ++g_cases;
            if (crc_sliced<W>(t, p, n) != crc_bitwise<W>(poly, p, n, 0))
                fail("crc tables", W, (long)n, rep, 0);
        }
    static const size_t kLenB[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 4095, 4096, 65535,
                                   65536, 65537, 100000, (1u << 17) - 1, 1u << 17};
    for (size_t nb : kLenB)
        for (size_t na = 0; na <= 70; na += 7) {
            const uint32_t ca = crc_bitwise<W>(poly, buf.data(), na, 0);
            const uint32_t cb = crc_bitwise<W>(poly, buf.data() + na, nb, 0);
            const uint32_t whole = crc_bitwise<W>(poly, buf.data() + na, nb, ca);
            ++g_cases;
            if ((advance<W>(adv, ca, nb) ^ cb) != whole)
                fail("crc advance", W, (long)na, (long)nb, 0);
        }
    for (int rep = 0; rep < 200; ++rep) {
        const size_t na = rnd() % 71, nb = rnd() % ((1u << 17) + 1);
        const uint32_t ca = crc_bitwise<W>(poly, buf.data(), na, 0);
        const uint32_t cb = crc_bitwise<W>(poly, buf.data() + na, nb, 0);
        ++g_cases;
        if ((advance<W>(adv, ca, nb) ^ cb) != crc_bitwise<W>(poly, buf.data() + na, nb, ca))
            fail("crc advance", W, (long)na, (long)nb, 1);
    }
}

// ---- the builders crc_common.h replaced, as they stood
namespace old_engine { // engine.hip build_crc_tables, without the advq part
void build(uint32_t t16[4][256], uint32_t *t8, uint16_t adv[24][16])
{
    for (uint32_t b = 0; b < 256; ++b) {
        uint32_t c = b << 8, c8 = b;
        for (int i = 0; i < 8; ++i) {
            c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) : (c << 1);
            c8 = (c8 & 0x80u) ? ((c8 << 1) ^ 0x07u) : (c8 << 1);
        }
        t16[0][b] = c & 0xFFFFu;
        t8[b] = c8 & 0xFFu;
    }
    for (int k = 1; k < 4; ++k)
        for (uint32_t b = 0; b < 256; ++b) {
            const uint32_t c = t16[k - 1][b];
            t16[k][b] = ((c << 8) ^ t16[0][(c >> 8) & 0xFFu]) & 0xFFFFu;
        }
    for (int i = 0; i < 16; ++i) {
        uint32_t s = 1u << i;
        s = ((s << 8) ^ t16[0][(s >> 8) & 0xFFu]) & 0xFFFFu;
        adv[0][i] = (uint16_t)s;
    }
    for (int m = 1; m < 24; ++m) {
        for (int i = 0; i < 16; ++i) {
            uint32_t v = adv[m - 1][i], r = 0;
            for (int j = 0; j < 16; ++j)
                if ((v >> j) & 1u)
                    r ^= adv[m - 1][j];
            adv[m][i] = (uint16_t)r;
        }
    }
}
} // namespace old_engine

namespace old_dec { // flac_decode.hip build_dec_tables, build_dec_adv
void build_dec_adv(const uint16_t t16[4][256], uint16_t adv[24][16])
{
    for (int i = 0; i < 16; ++i) {
        uint32_t c = 1u << i;
        c = ((c << 8) ^ t16[0][(c >> 8) & 0xFFu]) & 0xFFFFu;
        adv[0][i] = (uint16_t)c;
    }
    for (int m = 1; m < 24; ++m)
        for (int i = 0; i < 16; ++i) {
            uint32_t v = adv[m - 1][i], r = 0;
            for (int j = 0; j < 16; ++j)
                if ((v >> j) & 1u)
                    r ^= adv[m - 1][j];
            adv[m][i] = (uint16_t)r;
        }
}
void build_dec_tables(uint8_t *t8, uint16_t t16[4][256])
{
    for (uint32_t b = 0; b < 256; ++b) {
        uint32_t c8 = b;
        for (int i = 0; i < 8; ++i)
            c8 = (c8 & 0x80) ? ((c8 << 1) ^ 0x07) : (c8 << 1);
        t8[b] = (uint8_t)c8;
        uint32_t c = b << 8;
        for (int i = 0; i < 8; ++i)
            c = (c & 0x8000) ? ((c << 1) ^ 0x8005) : (c << 1);
        t16[0][b] = (uint16_t)c;
    }
    for (int k = 1; k < 4; ++k)
        for (uint32_t b = 0; b < 256; ++b) {
            const uint32_t p = t16[k - 1][b];
            t16[k][b] = (uint16_t)(((p << 8) & 0xFFFF) ^ t16[0][p >> 8]);
        }
}
} // namespace old_dec

namespace old_ogg { // ogg_demux.hip ogg_upload_tables
void build(uint32_t tab[4][256], uint32_t adv[17][32])
{
    for (uint32_t b = 0; b < 256; ++b) {
        uint32_t c = b << 24;
        for (int i = 0; i < 8; ++i)
            c = (c & 0x80000000u) ? (c << 1) ^ 0x04C11DB7u : c << 1;
        tab[0][b] = c;
    }
    for (int k = 1; k < 4; ++k)
        for (uint32_t b = 0; b < 256; ++b) {
            const uint32_t p = tab[k - 1][b];
            tab[k][b] = (p << 8) ^ tab[0][p >> 24];
        }
    for (int i = 0; i < 32; ++i) {
        const uint32_t c = 1u << i;
        adv[0][i] = (c << 8) ^ tab[0][c >> 24];
    }
    for (int m = 1; m < 17; ++m)
        for (int i = 0; i < 32; ++i) {
            const uint32_t v = adv[m - 1][i];
            uint32_t r = 0;
            for (int j = 0; j < 32; ++j)
                if ((v >> j) & 1u)
                    r ^= adv[m - 1][j];
            adv[m][i] = r;
        }
}
} // namespace old_ogg

static void same(const char *what, const void *a, const void *b, size_t n)
{
    ++g_cases;
    if (memcmp(a, b, n))
        fail(what, (long)n, 0, 0, 0);
}

static void check_old_tables()
{
    { // the encoder's: 32-bit CRC-16 and CRC-8 entries, 16-bit matrices
        static uint32_t t16[4][256], t8[256], n16[4][256], n8[256];
        static uint16_t adv[24][16], nadv[24][16];
        old_engine::build(t16, t8, adv);
        crc_build_tables<16>(0x8005u, &n16[0][0], 4);
        crc_build_tables<8>(0x07u, n8, 1);
        crc_build_advance<16>(n16[0], &nadv[0][0], 24);
        same("engine t16", t16, n16, sizeof(t16));
        same("engine t8", t8, n8, sizeof(t8));
        same("engine adv", adv, nadv, sizeof(adv));
    }
    { // the decoder's: 16-bit and 8-bit entries
        static uint16_t t16[4][256], n16[4][256], adv[24][16], nadv[24][16];
        static uint8_t t8[256], n8[256];
        old_dec::build_dec_tables(t8, t16);
        old_dec::build_dec_adv(t16, adv);
        crc_build_tables<8>(0x07u, n8, 1);
        crc_build_tables<16>(0x8005u, &n16[0][0], 4);
        crc_build_advance<16>(n16[0], &nadv[0][0], 24);
        same("decoder t16", t16, n16, sizeof(t16));
        same("decoder t8", t8, n8, sizeof(t8));
        same("decoder adv", adv, nadv, sizeof(adv));
    }
    { // Ogg's CRC-32
        static uint32_t tab[4][256], adv[17][32], ntab[4][256], nadv[17][32];
        old_ogg::build(tab, adv);
        crc_build_tables<32>(0x04C11DB7u, &ntab[0][0], 4);
        crc_build_advance<32>(ntab[0], &nadv[0][0], 17);
        same("ogg tables", tab, ntab, sizeof(tab));
        same("ogg adv", adv, nadv, sizeof(adv));
    }
}

int main()
{
    check_ranges<false>();
    check_ranges<true>();
    check_runs<false>();
    check_runs<true>();
    for (int op = 0; op < 5; ++op)
        for (int h = 0; h <= 64; ++h)
            if (!g_level[op][h])
                fail("fill level not met", op, h, 0, 0);
    const uint64_t reader_cases = g_cases;
    check_crc<16>(0x8005u);
    check_crc<32>(0x04C11DB7u);
    check_old_tables();
    printf("bits_crc_check: %llu reader cases, %llu crc cases, %llu failed\n",
           (unsigned long long)reader_cases, (unsigned long long)(g_cases - reader_cases),
           (unsigned long long)g_bad);
    return g_bad ? 1 : 0;
}
