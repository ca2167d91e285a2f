// audio_fir.h -- the kernels of audioSink's three interpolators, LowPassFIR (5, 16000, 48000),
// (5, 24000, 48000) and (5, 32000, 96000), as LowPassFIR's constructor computes them
// (fir-filters.cpp:35-69; audiosink.cpp:71-73): f, temp and sum are float, the sine, the Blackman
// window and their arguments double, each assignment rounding to float.  One definition for the
// library's host table (DABGPU_TABLE_AUDIO_FIR) and the host audioResampler.  <cmath> only.
#pragma once
#include <cmath>
#include <cstdint>

namespace dabgpu {

inline void audio_fir_kernels(float k[15]) {
    const int32_t Fc[3] = {16000, 24000, 32000}, fs[3] = {48000, 48000, 96000};
    const int16_t size = 5;
    for (int r = 0; r < 3; r++) {
        const float f = (float)Fc[r] / fs[r];
        float sum = 0.0, temp[5];
        for (int16_t i = 0; i < size; i++) {
            const int d = i - size / 2;
            if (d == 0) temp[i] = 2 * M_PI * f;
            else temp[i] = std::sin(2 * M_PI * f * d) / d;
            temp[i] *= (0.42 - 0.5 * std::cos(2 * M_PI * (float)i / size) + 0.08 * std::cos(4 * M_PI * (float)i / size));
            sum += temp[i];
        }
        for (int i = 0; i < size; i++) k[5 * r + i] = temp[i] / sum;
    }
}

}  // namespace dabgpu
