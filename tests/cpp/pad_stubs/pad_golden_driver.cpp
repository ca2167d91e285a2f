// Driver of tests/golden/make_pad_golden.py: ONE fixture per process (dynamicLabel keeps its
// state in function-local statics that outlive a handler), fed as mp4Processor feeds it
// (mp4processor.cpp:237-265): the AU copied into a zeroed theAU[1920], processPAD when its first
// element is a data stream element.  The padHandler is made by placement new in storage filled
// with the byte given on the command line; the generator runs every fixture with 0x00 and with
// 0xA5 and refuses to write the file unless both runs give the same records, which shows that
// no fixture reads a member nothing initialised.
//   input : int32 n_aus; per AU int32 length (negative: failed its CRC, not fed), int32 n_bytes, bytes
//   output: int32 n_labels; per label int32 au, charSet, n_pieces, n_bytes, the piece sizes
//           (int32 each), the pieces' charsets (int32 each), the bytes;
//           int32 n_calls; per process_mscGroup call int32 au, groupType, last, segmentNumber,
//           transportId, index (of the data pointer in the group buffer), length
//           (msc_dataGroupLength), then the buffer's first `length` bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>
#define private public
#include "pad-handler.h"
#undef private
#include "mot-data.h"

struct Label {
    int32_t au, charset;
    QString text;
};
static std::vector<Label> labels;
static int32_t cur_au;
static padHandler *handler;

void padHandler::showLabel(QString s) { labels.push_back(Label{cur_au, (int32_t)handler->charSet, s}); }

static std::vector<std::vector<int32_t>> calls;
static std::vector<std::string> call_bytes;
void pad_mot_call(const uint8_t *data, int groupType, int lastSegment, int segmentNumber, int transportId) {
    const int32_t index = (int32_t)(data - handler->msc_dataGroupBuffer), length = handler->msc_dataGroupLength;
    if (length < 0 || length > 8192) exit(5);
    calls.push_back({cur_au, groupType, lastSegment, segmentNumber, transportId, index, length});
    call_bytes.push_back(std::string((const char *)handler->msc_dataGroupBuffer, (size_t)length));
}

static void put(FILE *f, const std::vector<int32_t> &v) { fwrite(v.data(), sizeof(int32_t), v.size(), f); }

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const int fill = (int)strtol(argv[3], nullptr, 0);
    RadioInterface gui;
    void *storage = malloc(sizeof(padHandler));
    memset(storage, fill, sizeof(padHandler));
    handler = new (storage) padHandler(&gui);
    int32_t n_aus;
    if (fread(&n_aus, sizeof n_aus, 1, in) != 1) return 3;
    for (cur_au = 0; cur_au < n_aus; cur_au++) {
        int32_t h[2];
        if (fread(h, sizeof h, 1, in) != 1 || h[1] < 0) return 3;
        std::vector<uint8_t> src((size_t)h[1]);
        if (h[1] && fread(src.data(), 1, src.size(), in) != src.size()) return 3;
        if (h[0] < 0) continue;
        if (h[0] >= 960 || h[0] > h[1]) return 4;                    // (mp4processor.cpp:248)
        uint8_t *theAU = new uint8_t[2 * 960];
        memset(theAU, 0, 2 * 960);
        memcpy(theAU, src.data(), (size_t)h[0]);
        if (((theAU[0] >> 5) & 07) == 4) handler->processPAD(theAU);
        delete[] theAU;
    }
    put(out, {(int32_t)labels.size()});
    for (auto &l : labels) {
        put(out, {l.au, l.charset, (int32_t)l.text.pieces.size(), (int32_t)l.text.bytes.size()});
        put(out, l.text.pieces);
        put(out, l.text.charsets);
        fwrite(l.text.bytes.data(), 1, l.text.bytes.size(), out);
    }
    put(out, {(int32_t)calls.size()});
    for (size_t k = 0; k < calls.size(); k++) {
        put(out, calls[k]);
        fwrite(call_bytes[k].data(), 1, call_bytes[k].size(), out);
    }
    fclose(out);
    handler->~padHandler();
    free(storage);
    return 0;
}
