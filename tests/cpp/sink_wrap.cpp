// TEST INFRASTRUCTURE: a C surface over the host audioResampler (msc_consumers.h) so that
// tests/test_sink_cpu.py can drive it from Python (ctypes) and compare it with tests/sink_py.py
// and the golden file.
#include <cstring>
#include <vector>

#include "msc_consumers.h"

extern "C" {

void *sw_new(void) { return new dabgpu::audioResampler(); }
void sw_free(void *h) { delete static_cast<dabgpu::audioResampler *>(h); }
// one audioOut call: returns the pairs delivered (copied to out, at most max_pairs of them), -1 for
// a refused call
int sw_audio_out(void *h, const int16_t *pcm, int amount, int rate, float *out, int max_pairs) {
    std::vector<float> v;
    if (!static_cast<dabgpu::audioResampler *>(h)->audioOut(pcm, amount, rate, v)) return -1;
    const int n = (int)(v.size() / 2);
    if (n) std::memcpy(out, v.data(), sizeof(float) * 2 * (size_t)(n < max_pairs ? n : max_pairs));
    return n;
}
void sw_kernels(float *out15) { std::memcpy(out15, dabgpu::audioResampler::kernels(), 15 * sizeof(float)); }

}
