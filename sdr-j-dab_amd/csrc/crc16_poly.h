// crc16_poly.h -- CRC-16-CCITT (x^16 + x^12 + x^5 + 1) as arithmetic on polynomials over GF(2)
// modulo P, for the kernels that take a CRC in slices (the CRC is linear: a slice's register
// from zero, times x^(8 * bytes after it), xor over the slices, plus the preset's share).
// No HIP in here: a host compiler takes the header alone (tests/cpp/test_crc16_poly.cpp).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define CRC16_FN __host__ __device__ constexpr
#else
#define CRC16_FN constexpr
#endif

namespace dab {
namespace crc16 {

CRC16_FN uint32_t mulmod(uint32_t a, uint32_t b) {       // a * b mod P (a, b < 2^16)
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x11021u;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
CRC16_FN uint32_t xpow8(int n) {                         // x^(8 n) mod P
    uint32_t r = 1, b = 0x100;
    for (; n; n >>= 1) {
        if (n & 1) r = mulmod(r, b);
        b = mulmod(b, b);
    }
    return r;
}
// the register after one more byte (the message times x^16, from whatever it held)
CRC16_FN uint32_t crc_byte(uint32_t crc, uint32_t b) {
    crc = ((crc >> 8) | (crc << 8)) & 0xFFFFu;
    crc ^= b;
    crc ^= (crc & 0xFFu) >> 4;
    crc ^= (crc << 12) & 0xFFFFu;
    crc ^= (crc & 0xFFu) << 5;
    return crc;
}
// the all-ones preset's share of the register after nbytes bytes
CRC16_FN uint32_t crc_ones(int nbytes) { return mulmod(0xFFFFu, xpow8(nbytes)); }
// check_CRC_bits inverts the last 16 bits and wants a zero register: the register over the
// bytes as they are (from zero, plus crc_ones of their count) must equal 0xFFFF * x^16
constexpr uint32_t CRC_GOOD = mulmod(0xFFFFu, 0x1021u);

}  // namespace crc16
}  // namespace dab
