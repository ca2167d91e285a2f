// Driver of tests/golden/make_mp2_golden.py: one mp2Processor per stream, the stream's bits
// through addtoFrame in CIF-sized pieces, what reaches the sink written out.
//   input : per stream  int32 bitRate, int32 n_bits, n_bits bytes (one bit each)
//   output: per stream  int32 n_frames, then per frame int32 rate, int16 pcm[2304]
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mp2processor.h"
#include "gui.h"

// what the decoder's translation unit leaves to the rest of the receiver
void mp2Processor::show_successRate(int) {}
dabProcessor::dabProcessor(void) {}
dabProcessor::~dabProcessor(void) {}
void dabProcessor::addtoFrame(uint8_t *, int16_t) {}
void dabProcessor::setFile(FILE *) {}
void dabProcessor::stop(void) {}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t hdr[2];
    while (fread(hdr, sizeof hdr, 1, in) == 1) {
        std::vector<uint8_t> bits(hdr[1]);
        if (fread(bits.data(), 1, bits.size(), in) != bits.size()) return 3;
        RadioInterface gui;
        audioSink sink;
        mp2Processor proc(&gui, &sink, NULL, (int16_t)hdr[0]);
        const int cif = 24 * hdr[0];
        for (size_t p = 0; p + cif <= bits.size(); p += cif) proc.addtoFrame(bits.data() + p, (int16_t)cif);
        const int32_t n = (int32_t)sink.rate.size();
        fwrite(&n, sizeof n, 1, out);
        for (int32_t k = 0; k < n; k++) {
            fwrite(&sink.rate[k], sizeof(int32_t), 1, out);
            fwrite(sink.pcm.data() + (size_t)k * 2304, sizeof(int16_t), 2304, out);
        }
    }
    fclose(out);
    return 0;
}
