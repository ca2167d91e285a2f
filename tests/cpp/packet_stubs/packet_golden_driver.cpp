// Driver of tests/golden/make_packet_golden.py: per fixture two mscDatagroup objects (show_crcErrors
// on), one with the plain handler (DSCTy 5, DG flag 0: every group recorded as it is handed
// over) and one with the MOT builder (DSCTy 60: what reaches motHandler::process_mscGroup),
// fed through handlePackets in CIF-sized pieces.
//   input : per fixture  int32 bitRate, int32 n_cif, n_cif * 3 * bitRate bytes
//   output: per fixture  int32 n_groups, per group int32 n_bytes + bytes;
//                        int32 n_quality + int32 values;  int32 n_mot + 4 int32 each
#include <cstdio>
#include <cstdlib>
#include <vector>
#define private public
#include "msc-datagroup.h"
#undef private
#include "virtual-datahandler.h"
#include "mot-data.h"
#include "gui.h"

std::vector<motCall> mot_calls;
static std::vector<std::vector<uint8_t>> groups;
static std::vector<int32_t> quality;

// what the two translation units leave to the rest of the receiver
void mscDatagroup::show_mscErrors(int v) { quality.push_back(v); }
virtual_dataHandler::virtual_dataHandler(void) {}
virtual_dataHandler::~virtual_dataHandler(void) {}
void virtual_dataHandler::add_mscDatagroup(QByteArray &msc) {       // the recording handler
    std::vector<uint8_t> g(msc.size() / 8);
    for (size_t i = 0; i < g.size(); i++) g[i] = (uint8_t)getBits_8((uint8_t *)msc.data(), (int16_t)(8 * i));
    groups.push_back(g);
}
dabVirtual::dabVirtual(void) {}
dabVirtual::~dabVirtual(void) {}
int32_t dabVirtual::process(int16_t *, int16_t) { return 0; }
void dabVirtual::stopRunning(void) {}
void dabVirtual::stop(void) {}
void dabVirtual::setFiles(FILE *, FILE *) {}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t hdr[2];
    RadioInterface gui;
    while (fread(hdr, sizeof hdr, 1, in) == 1) {
        const int nb = 3 * hdr[0];
        std::vector<uint8_t> rows((size_t)hdr[1] * nb);
        if (fread(rows.data(), 1, rows.size(), in) != rows.size()) return 3;
        groups.clear();
        quality.clear();
        mot_calls.clear();
        for (int pass = 0; pass < 2; pass++) {
            mscDatagroup dg(&gui, pass ? 60 : 5, 0, 6, (int16_t)hdr[0], 1, 2, 0, 0, true);
            std::vector<uint8_t> bits(8 * nb);
            for (int c = 0; c < hdr[1]; c++) {
                for (int i = 0; i < 8 * nb; i++) bits[i] = (rows[(size_t)c * nb + (i >> 3)] >> (7 - (i & 7))) & 1;
                dg.handlePackets(bits.data(), (int16_t)(8 * nb));
            }
            if (pass == 0) quality.clear();          // (the second pass emits the same values)
        }
        int32_t n = (int32_t)groups.size();
        fwrite(&n, sizeof n, 1, out);
        for (auto &g : groups) {
            n = (int32_t)g.size();
            fwrite(&n, sizeof n, 1, out);
            fwrite(g.data(), 1, g.size(), out);
        }
        n = (int32_t)quality.size();
        fwrite(&n, sizeof n, 1, out);
        fwrite(quality.data(), sizeof(int32_t), quality.size(), out);
        n = (int32_t)mot_calls.size();
        fwrite(&n, sizeof n, 1, out);
        fwrite(mot_calls.data(), sizeof(motCall), mot_calls.size(), out);
    }
    fclose(out);
    return 0;
}
