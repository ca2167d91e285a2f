// rate_converter.h -- the input rate conversion of airspyHandler (airspy-handler.cpp:138-148,
// 333-359) without a device: samples at rate Hz in, 2.048 MHz cf32 out, bit for bit what
// dabgpu_rate_convert (k_rate.hip) writes.  HIP-free and header-only: the library's context builds
// its device tables with rate_tables, CPU-only users and the tests use rateConverter.
//
// With M = rate / 1000 the handler collects M + 1 samples (convBuffer), writes 2048 outputs
//   out[j] = conv[base[j] + 1] * frac[j] + conv[base[j]] * (1.0f - frac[j])      (re and im alike)
// and carries conv[M] over as conv[0] of the next block.  Every product, the 1.0f - frac and the
// sum round to fp32 on their own: whatever includes this header is built with -ffp-contract=off.
#pragma once
#include <cmath>
#include <complex>
#include <cstdint>
#include <vector>

namespace dabgpu {

// the sample formats of include/dabgpu.h (DABGPU_IQ_*), restated so that this header needs no other
enum { RATE_IQ_F32 = 0, RATE_IQ_U8 = 1, RATE_IQ_S16 = 2, RATE_IQ_S12 = 3 };

// rates the converter takes: whole kHz from the output rate up to 10 MHz
inline bool rate_valid(int rate) { return rate >= 2048000 && rate <= 10000000 && rate % 1000 == 0; }
inline bool rate_format_valid(int format) { return format >= RATE_IQ_F32 && format <= RATE_IQ_S12; }
inline int rate_format_bytes(int format) { return format == RATE_IQ_F32 ? 8 : format == RATE_IQ_U8 ? 2 : 4; }   // per I/Q pair

// mapTable_int and mapTable_float as the handler's constructor computes them (airspy-handler.cpp:
// 142-146): the quotient and the product in double, the difference rounded once to float.  (All of
// it is exact: M / 2048 and j * M / 2048 need 35 bits at most, the fraction 11.)
inline void rate_tables(int rate, int16_t *base, float *frac) {
    const float inVal = float(rate / 1000);
    for (int j = 0; j < 2048; j++) {
        base[j] = (int16_t) int(std::floor(j * (inVal / 2048.0)));
        frac[j] = (float)(j * (inVal / 2048.0) - base[j]);
    }
}

// one sample of a stream in `format` as the float pair the interpolation reads
inline std::complex<float> rate_sample(int format, const void *src, int64_t i) {
    switch (format) {
    case RATE_IQ_S12: {       // airspy-handler.cpp:340-341
        const int16_t *p = (const int16_t *)src + 2 * i;
        return {p[0] / (float)2048, p[1] / (float)2048};
    }
    case RATE_IQ_S16: {       // wavfiles.cpp:172 (sf_readf_float)
        const int16_t *p = (const int16_t *)src + 2 * i;
        return {p[0] / 32768.0f, p[1] / 32768.0f};
    }
    case RATE_IQ_U8: {        // rawfiles.cpp:115-117
        const uint8_t *p = (const uint8_t *)src + 2 * i;
        return {(float)(p[0] - 128) / 128.0f, (float)(p[1] - 128) / 128.0f};
    }
    default: {
        const float *p = (const float *)src + 2 * i;
        return {p[0], p[1]};
    }
    }
}

class rateConverter {
public:
    typedef std::complex<float> DSPCOMPLEX;
    // rate and format as rate_valid / rate_format_valid accept them (anything else: ok() is false
    // and convert delivers nothing)
    rateConverter(int rate, int format)
        : ok_(rate_valid(rate) && rate_format_valid(format)), format_(format), convBufferSize(ok_ ? rate / 1000 : 0), convIndex(0),
          convBuffer((size_t)convBufferSize + 1), mapTable_int(2048), mapTable_float(2048) {
        if (ok_) rate_tables(rate, mapTable_int.data(), mapTable_float.data());
    }
    bool ok() const { return ok_; }
    int block() const { return convBufferSize; }                       // M: input samples per 2048 outputs
    const int16_t *table_int() const { return mapTable_int.data(); }   // [2048]
    const float *table_float() const { return mapTable_float.data(); } // [2048]
    // n samples in, the completed blocks appended to out: returns how many samples that were.
    // Any chunking of a stream gives the same output.
    int64_t convert(const void *src, int64_t n, std::vector<DSPCOMPLEX> &out) {
        int64_t made = 0;
        if (!ok_) return 0;
        for (int64_t i = 0; i < n; i++) {
            convBuffer[convIndex++] = rate_sample(format_, src, i);
            if (convIndex <= convBufferSize) continue;
            const size_t at = out.size();
            out.resize(at + 2048);
            for (int j = 0; j < 2048; j++) {
                const DSPCOMPLEX a = convBuffer[mapTable_int[j] + 1], b = convBuffer[mapTable_int[j]];
                const float r = mapTable_float[j], q = 1.0f - r;
                out[at + j] = DSPCOMPLEX(a.real() * r + b.real() * q, a.imag() * r + b.imag() * q);
            }
            made += 2048;
            convBuffer[0] = convBuffer[convBufferSize];     // the last sample starts the next block
            convIndex = 1;
        }
        return made;
    }
    // forget the samples held: the next sample is a stream's first
    void reset() { convIndex = 0; }

private:
    bool ok_;
    int format_;
    int convBufferSize, convIndex;
    std::vector<DSPCOMPLEX> convBuffer;
    std::vector<int16_t> mapTable_int;
    std::vector<float> mapTable_float;
};

}  // namespace dabgpu
