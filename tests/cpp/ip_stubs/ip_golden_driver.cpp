// Driver of tests/golden/make_ip_golden.py: one ip_dataHandler (show_crcErrors on), fed one
// fixture's data groups as mscDatagroup hands them over: a QByteArray of bits, one per byte, of
// exactly the group's length.  Records every writeDatagram and show_ipErrors (defined here: the
// signals have no moc) with the call that made it.
//   input : int32 n_calls; per call int32 n_bytes, then the bytes
//   output: int32 n_events; per event int32 call, kind (0 datagram, 1 show_ipErrors), value
//           (the datagram's length, or the emitted number), then a datagram's bytes
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ip-datahandler.h"
#include "gui.h"

struct Event {
    int32_t call, kind, value;
    std::string bytes;
};
static std::vector<Event> events;
static int32_t cur_call;

void ip_dataHandler::writeDatagram(char *d, int n) {
    if (n < 0) { fprintf(stderr, "writeDatagram with length %d\n", n); abort(); }
    events.push_back(Event{cur_call, 0, n, std::string(d, (size_t)n)});
}
void ip_dataHandler::show_ipErrors(int v) { events.push_back(Event{cur_call, 1, v, std::string()}); }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    RadioInterface gui;
    int32_t n_calls;
    if (fread(&n_calls, sizeof n_calls, 1, in) != 1) return 3;
    ip_dataHandler *h = new ip_dataHandler(&gui, true);
    for (cur_call = 0; cur_call < n_calls; cur_call++) {
        int32_t n;
        if (fread(&n, sizeof n, 1, in) != 1 || n < 0) return 3;
        std::vector<uint8_t> bytes((size_t)n);
        if (n && fread(bytes.data(), 1, (size_t)n, in) != (size_t)n) return 3;
        QByteArray msc;
        msc.resize(8 * n);
        for (int i = 0; i < 8 * n; i++) msc[i] = (char)((bytes[(size_t)(i >> 3)] >> (7 - (i & 7))) & 1);
        h->add_mscDatagroup(msc);
    }
    delete h;
    int32_t n = (int32_t)events.size();
    fwrite(&n, sizeof n, 1, out);
    for (auto &e : events) {
        int32_t r[3] = {e.call, e.kind, e.value};
        fwrite(r, sizeof r, 1, out);
        fwrite(e.bytes.data(), 1, e.bytes.size(), out);
    }
    fclose(out);
    fclose(in);
    return 0;
}
