// Driver of tests/golden/make_sink_golden.py: the kernels of the three LowPassFIR objects audioSink
// constructs, then one audioSink per scripted sequence, every call through audioOut and what
// arrived in _O_Buffer (capacity () before and after) drained through paCallback_o.
//   input : per sink  int32 n_calls, then per call int32 rate, int32 amount, int16 pcm[2 * amount]
//   output: float coef[3][5]; per call int32 n_pairs, float samples[2 * n_pairs]
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "audiosink.h"

// one silent device; the stream is a flag that says whether it runs
static const PaHostApiInfo kApi = {"none"};
static const PaDeviceInfo kDev = {"null", 0, 2, 0.0, 0.0};
static int running = 0;
PaError Pa_Initialize(void) { return paNoError; }
PaError Pa_Terminate(void) { return paNoError; }
PaHostApiIndex Pa_GetHostApiCount(void) { return 1; }
const PaHostApiInfo *Pa_GetHostApiInfo(PaHostApiIndex) { return &kApi; }
PaDeviceIndex Pa_GetDeviceCount(void) { return 1; }
PaDeviceIndex Pa_GetDefaultOutputDevice(void) { return 0; }
const PaDeviceInfo *Pa_GetDeviceInfo(PaDeviceIndex) { return &kDev; }
PaError Pa_IsFormatSupported(const PaStreamParameters *, const PaStreamParameters *, double) { return paFormatIsSupported; }
PaError Pa_OpenStream(PaStream **s, const PaStreamParameters *, const PaStreamParameters *, double, unsigned long, unsigned long,
                      PaStreamCallback *, void *) {
    *s = &running;
    return paNoError;
}
PaError Pa_CloseStream(PaStream *) { return paNoError; }
PaError Pa_StartStream(PaStream *) { running = 1; return paNoError; }
PaError Pa_StopStream(PaStream *) { running = 0; return paNoError; }
PaError Pa_AbortStream(PaStream *) { running = 0; return paNoError; }
PaError Pa_IsStreamStopped(PaStream *) { return !running; }
void Pa_Sleep(long) {}
sf_count_t sf_writef_float(SNDFILE *, const float *, sf_count_t frames) { return frames; }

class drainedSink : public audioSink {
public:
    explicit drainedSink(QComboBox *s) : audioSink(s) {}
    void drain(float *out, unsigned long n_pairs) { (void)paCallback_o(NULL, out, n_pairs, NULL, 0, this); }
};

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const int32_t Fc[3] = {16000, 24000, 32000}, fs[3] = {48000, 48000, 96000};
    for (int r = 0; r < 3; r++) {
        LowPassFIR f(5, Fc[r], fs[r]);
        for (int i = 0; i < 5; i++) {                 // the impulse response of Pass (DSPFLOAT) is the kernel
            const float k = f.Pass(i == 0 ? 1.0f : 0.0f);
            fwrite(&k, sizeof k, 1, out);
        }
    }
    int32_t n_calls;
    while (fread(&n_calls, sizeof n_calls, 1, in) == 1) {
        QComboBox box;
        drainedSink sink(&box);
        if (!sink.selectDefaultDevice()) return 4;
        for (int32_t c = 0; c < n_calls; c++) {
            int32_t hdr[2];
            if (fread(hdr, sizeof hdr, 1, in) != 1 || hdr[1] < 0 || hdr[1] > 32768) return 3;
            std::vector<int16_t> pcm(2 * (size_t)hdr[1] + 2);
            if (hdr[1] && fread(pcm.data(), 2 * sizeof(int16_t), hdr[1], in) != (size_t)hdr[1]) return 3;
            const int32_t before = sink.capacity();
            sink.audioOut(pcm.data(), hdr[1], hdr[0]);
            const int32_t n = before - sink.capacity();
            std::vector<float> got(2 * (size_t)n + 2);
            sink.drain(got.data(), (unsigned long)n);
            if (sink.capacity() != before) return 5;
            fwrite(&n, sizeof n, 1, out);
            fwrite(got.data(), 2 * sizeof(float), n, out);
        }
    }
    fclose(out);
    return 0;
}
