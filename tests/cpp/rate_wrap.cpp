// TEST INFRASTRUCTURE: a C surface over the host rateConverter (rate_converter.h) so that
// tests/test_rate_cpu.py and the GPU tests can drive it from Python (ctypes) and compare it with
// the golden file and with dabgpu_rate_convert.
#include <cstring>
#include <vector>

#include "rate_converter.h"

extern "C" {

// null for a rate or format the converter does not take
void *rw_new(int rate, int format) {
    dabgpu::rateConverter *c = new dabgpu::rateConverter(rate, format);
    if (c->ok()) return c;
    delete c;
    return nullptr;
}
void rw_free(void *h) { delete static_cast<dabgpu::rateConverter *>(h); }
int rw_block(void *h) { return static_cast<dabgpu::rateConverter *>(h)->block(); }
void rw_tables(void *h, int16_t *base, float *frac) {
    std::memcpy(base, static_cast<dabgpu::rateConverter *>(h)->table_int(), 2048 * sizeof(int16_t));
    std::memcpy(frac, static_cast<dabgpu::rateConverter *>(h)->table_float(), 2048 * sizeof(float));
}
// n samples in: returns the output samples completed (copied to out, at most max_out of them)
long long rw_convert(void *h, const void *src, long long n, float *out, long long max_out) {
    std::vector<dabgpu::rateConverter::DSPCOMPLEX> v;
    const long long made = static_cast<dabgpu::rateConverter *>(h)->convert(src, n, v);
    if (made) std::memcpy(out, v.data(), sizeof(float) * 2 * (size_t)(made < max_out ? made : max_out));
    return made;
}

}
