// The kernels' CRC-16-CCITT arithmetic (sdr-j-dab_amd/csrc/crc16_poly.h) against a CRC taken one
// bit at a time as check_CRC_bits defines it (dab-constants.h): a 16-bit register preset to all
// ones, the message's bits msb first with the last 16 inverted, generator x^16 + x^12 + x^5 + 1,
// and the message passes when the register ends at zero.  The 64-slice combination is done here
// in plain C++ with the slice bounds wave_crc16 (msc_feed.h) uses.  Host code only: the header
// needs no GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "crc16_poly.h"

using namespace dab::crc16;

// the values the three kernels' own constants had before they shared this header
static_assert(CRC_GOOD == 0x1D0Fu, "0xFFFF * x^16 mod P");
static_assert(xpow8(24) == 0x650Bu, "x^192 mod P: one 24-byte cell further");
static_assert(crc_ones(24) == 0xEF8Au && crc_ones(48) == 0xDF9Du && crc_ones(72) == 0x040Eu && crc_ones(96) == 0x8A2Cu,
              "the all-ones preset after a packet of 1..4 cells");
static_assert(xpow8(0) == 1u && xpow8(1) == 0x100u && xpow8(2) == 0x1021u && crc_ones(0) == 0xFFFFu, "small powers");

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            if (fails++ < 20) printf("%s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                            \
    } while (0)

// check_CRC_bits over the bytes' bits, msb first
static bool bitwise_ok(const std::vector<uint8_t> &m) {
    const size_t nbits = 8 * m.size();
    if (nbits < 16) return false;
    uint32_t reg = 0xFFFFu;
    for (size_t i = 0; i < nbits; i++) {
        uint32_t bit = (m[i >> 3] >> (7 - (i & 7))) & 1u;
        if (i + 16 >= nbits) bit ^= 1u;
        const uint32_t top = (reg >> 15) & 1u;
        reg = (reg << 1) & 0xFFFFu;
        if (top ^ bit) reg ^= 0x1021u;
    }
    return reg == 0;
}
// the trailer that makes body + trailer pass: the complement of the register after the body
static uint32_t bitwise_trailer(const std::vector<uint8_t> &body) {
    uint32_t reg = 0xFFFFu;
    for (size_t i = 0; i < 8 * body.size(); i++) {
        const uint32_t bit = (body[i >> 3] >> (7 - (i & 7))) & 1u, top = (reg >> 15) & 1u;
        reg = (reg << 1) & 0xFFFFu;
        if (top ^ bit) reg ^= 0x1021u;
    }
    return ~reg & 0xFFFFu;
}

// the header's straight run: the register from zero over the bytes as they are, plus the preset's share
static uint32_t straight(const std::vector<uint8_t> &m) {
    uint32_t r = 0;
    for (uint8_t b : m) r = crc_byte(r, b);
    return r ^ crc_ones((int)m.size());
}
// ... and in 64 slices, as a wave takes it
static uint32_t sliced(const std::vector<uint8_t> &m) {
    const int n = (int)m.size(), per = (n + 63) / 64;
    uint32_t x = 0;
    for (int lane = 0; lane < 64; lane++) {
        const int a = std::min(n, lane * per), z = std::min(n, a + per);
        uint32_t part = 0;
        for (int i = a; i < z; i++) part = crc_byte(part, m[i]);
        x ^= mulmod(part, xpow8(n - z));
    }
    return x ^ crc_ones(n);
}

// a * b mod P by shift and reduce: a * x^i reduced step by step, summed over b's bits
static uint32_t slow_mulmod(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 0; i < 16; i++) {
        if ((b >> i) & 1u) r ^= a;
        a <<= 1;
        if (a & 0x10000u) a ^= 0x11021u;
    }
    return r;
}

int main() {
    std::mt19937 rng(20240611);
    // the verdicts and the slices
    const int sizes[] = {0, 1, 2, 3, 23, 24, 25, 63, 64, 65, 127, 128, 8191, 8192};
    for (int n : sizes) {
        std::vector<uint8_t> m(n);
        for (auto &b : m) b = (uint8_t)rng();
        CHECK(sliced(m) == straight(m));
        if (n < 2) {                                     // no room for a trailer: nothing passes
            CHECK(!bitwise_ok(m));
            continue;
        }
        std::vector<uint8_t> body(m.begin(), m.end() - 2);
        const uint32_t t = bitwise_trailer(body);
        m[n - 2] = (uint8_t)(t >> 8);
        m[n - 1] = (uint8_t)t;
        CHECK(bitwise_ok(m));
        CHECK(straight(m) == CRC_GOOD);
        CHECK(sliced(m) == CRC_GOOD);
        for (int k = 0; k < 16; k++) {                   // one flipped bit of the trailer, each in turn
            std::vector<uint8_t> w = m;
            w[n - 2 + k / 8] ^= (uint8_t)(0x80u >> (k % 8));
            CHECK(!bitwise_ok(w));
            CHECK(straight(w) != CRC_GOOD);
            CHECK(sliced(w) == straight(w));
        }
        if (n > 2) {                                     // ... and one of the body
            std::vector<uint8_t> w = m;
            w[rng() % (n - 2)] ^= (uint8_t)(1u << (rng() % 8));
            CHECK(!bitwise_ok(w));
            CHECK(straight(w) != CRC_GOOD);
            CHECK(sliced(w) == straight(w));
        }
    }
    // the multiply: every a against the 16 single-bit b and 256 random b
    std::vector<uint32_t> bs;
    for (int i = 0; i < 16; i++) bs.push_back(1u << i);
    for (int i = 0; i < 256; i++) bs.push_back(rng() & 0xFFFFu);
    long bad = 0;
    for (uint32_t a = 0; a < 0x10000u; a++)
        for (uint32_t b : bs) bad += mulmod(a, b) != slow_mulmod(a, b);
    CHECK(bad == 0);
    // xpow8 against repeated multiplication by x^8
    uint32_t p = 1;
    for (int n = 0; n <= 8192; n++) {
        if (n == 0 || n == 1 || n == 24 || n == 1023 || n == 8191 || n == 8192) CHECK(xpow8(n) == p);
        p = slow_mulmod(p, 0x100u);
    }
    if (fails) {
        printf("CRC16 POLY: %d checks failed\n", fails);
        return 1;
    }
    printf("CRC16 POLY OK\n");
    return 0;
}
