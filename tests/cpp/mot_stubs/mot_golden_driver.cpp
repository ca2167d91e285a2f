// Driver of tests/golden/make_mot_golden.py: per fixture one motHandler, fed the calls
// mot_databuilder::add_mscDatagroup would make, each with its data in a heap block of exactly
// the data field's length (so the address sanitizer sees every read past it).  Records what
// motHandler delivers: the_picture (defined here: the signal has no moc), and the files
// handleComplete writes into the working directory, which the driver collects after each call.
//   input : per fixture  int32 n_calls; per call int32 groupType, last, segmentNumber,
//                        transportId, n_bytes, then the bytes
//   output: per fixture  int32 n_events; per event int32 call, kind (1 slide, 3 file),
//                        contentsubType (slides), name length, body length, name, body
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dirent.h>
#include <string>
#include <unistd.h>
#include <vector>
#include "dab-constants.h"      // (its standard headers, before private is redefined)
#define private public
#include "mot-data.h"
#undef private
#include "gui.h"

struct Event {
    int32_t call, kind, subtype;
    std::string name, body;
};
static std::vector<Event> events;
static int32_t cur_call;

void motHandler::the_picture(QByteArray b, int subtype) {
    events.push_back(Event{cur_call, 1, subtype, std::string(), std::string(b.data(), (size_t)b.size())});
}

static void collect_files() {
    DIR *d = opendir(".");
    if (!d) exit(4);
    std::vector<std::string> names;
    while (dirent *e = readdir(d))
        if (strcmp(e->d_name, ".") && strcmp(e->d_name, "..")) names.push_back(e->d_name);
    closedir(d);
    for (auto &n : names) {
        FILE *f = fopen(n.c_str(), "rb");
        if (!f) exit(4);
        std::string body;
        char buf[4096];
        for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) body.append(buf, k);
        fclose(f);
        unlink(n.c_str());
        events.push_back(Event{cur_call, 3, 0, n, body});
    }
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out || chdir(argv[3])) return 2;
    RadioInterface gui;
    int32_t n_calls;
    while (fread(&n_calls, sizeof n_calls, 1, in) == 1) {
        motHandler *h = new motHandler(&gui);
        events.clear();
        for (cur_call = 0; cur_call < n_calls; cur_call++) {
            int32_t c[5];
            if (fread(c, sizeof c, 1, in) != 1) return 3;
            uint8_t *data = new uint8_t[(size_t)c[4]];
            if (c[4] && fread(data, 1, (size_t)c[4], in) != (size_t)c[4]) return 3;
            const size_t before = events.size();
            h->process_mscGroup(data, (uint8_t)c[0], c[1] != 0, (int16_t)c[2], (uint16_t)c[3]);
            if (events.size() > before) events.back().name = h->old_slide->name.s;   // show_slide has set it
            collect_files();
            delete[] data;
        }
        delete h;
        int32_t n = (int32_t)events.size();
        fwrite(&n, sizeof n, 1, out);
        for (auto &e : events) {
            int32_t r[5] = {e.call, e.kind, e.subtype, (int32_t)e.name.size(), (int32_t)e.body.size()};
            fwrite(r, sizeof r, 1, out);
            fwrite(e.name.data(), 1, e.name.size(), out);
            fwrite(e.body.data(), 1, e.body.size(), out);
        }
    }
    fclose(out);
    return 0;
}
