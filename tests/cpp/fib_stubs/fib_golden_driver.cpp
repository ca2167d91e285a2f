// TEST INFRASTRUCTURE: drives the reference's own fib_processor (src/backend/fib-processor.cpp,
// compiled where it lies by tests/golden/make_fib_golden.py against the stand-in headers of this
// directory) over one fixture's FIBs and writes what it signalled and what its lookups answer.
// The signals' bodies stand where moc's would: they record.  `new` fills what it hands out with a
// byte given on the command line: fib_processor's constructor leaves most of its 64 service
// entries' members to chance, and the generator runs every fixture with two fills to see which
// answers depend on that.
//
// usage: fib_golden IN OUT FILL
//   IN:  int32 n, then n FIBs of 32 bytes (msb first)
//   OUT: int32 n_signals, each {fib, kind (1 nameofEnsemble, 2 addtoEnsemble), id, n_pieces,
//        {size, charset} per piece, nbytes, bytes}; int32 n_named, each {slot, n_pieces, {size,
//        charset} per piece, nbytes, bytes, kindofService, audiodata as 9 int32, packetdata as 10
//        int32} (the structures start out as -7777 in every field)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

static int g_fill = 0;
void *operator new[](size_t n) {
    void *p = std::malloc(n ? n : 1);
    if (!p) throw std::bad_alloc();
    std::memset(p, g_fill, n);
    return p;
}
void operator delete[](void *p) noexcept { std::free(p); }
void operator delete[](void *p, size_t) noexcept { std::free(p); }

#define private public
#include "fib-processor.h"
#undef private
#include "gui.h"

struct sig {
    int fib, kind, id;
    QString s;
};
static std::vector<sig> g_sigs;
static int g_fib = 0;

void fib_processor::addEnsembleChar(char, int) {}
void fib_processor::addtoEnsemble(const QString &s) { g_sigs.push_back({g_fib, 2, 0, s}); }
void fib_processor::nameofEnsemble(int id, const QString &s) { g_sigs.push_back({g_fib, 1, id, s}); }
void fib_processor::technicalData(int, int, int, int, int, int, int) {}

static void put(std::FILE *f, int v) {
    const int32_t x = v;
    std::fwrite(&x, 4, 1, f);
}
static void put(std::FILE *f, const QString &s) {
    put(f, (int)s.pieces.size());
    for (size_t i = 0; i < s.pieces.size(); i++) {
        put(f, s.pieces[i]);
        put(f, s.charsets[i]);
    }
    put(f, (int)s.bytes.size());
    std::fwrite(s.bytes.data(), 1, s.bytes.size(), f);
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    g_fill = (int)std::strtol(argv[3], nullptr, 0);
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t n = 0;
    if (std::fread(&n, 4, 1, in) != 1 || n < 0 || n > 100000) return 3;
    std::vector<uint8_t> fibs((size_t)n * 32);
    if (n && std::fread(fibs.data(), 32, (size_t)n, in) != (size_t)n) return 3;
    std::fclose(in);
    RadioInterface radio;
    fib_processor *p = new fib_processor(&radio);
    // the FIC buffer of the reference's ficHandler holds a whole FIC block; here each FIB stands
    // alone in exactly 256 bytes on the heap, so that a read past it is the sanitizer's to report
    for (int i = 0; i < n; i++) {
        uint8_t *bits = (uint8_t *)std::malloc(256);
        for (int k = 0; k < 256; k++) bits[k] = (fibs[(size_t)i * 32 + (k >> 3)] >> (7 - (k & 7))) & 1;
        g_fib = i;
        p->process_FIB(bits, 0);
        std::free(bits);
    }
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    put(out, (int)g_sigs.size());
    for (const sig &s : g_sigs) {
        put(out, s.fib);
        put(out, s.kind);
        put(out, s.id);
        put(out, s.s);
    }
    std::vector<int> named;
    for (int i = 0; i < 64; i++)
        if (p->listofServices[i].inUse && p->listofServices[i].serviceLabel.hasName) named.push_back(i);
    put(out, (int)named.size());
    for (int i : named) {
        QString q = p->listofServices[i].serviceLabel.label;
        put(out, i);
        put(out, q);
        put(out, (int)p->kindofService(q));
        audiodata a;
        packetdata d;
        a.subchId = a.startAddr = a.protLevel = a.length = a.bitRate = a.ASCTy = a.language = a.programType = -7777;
        a.uepFlag = 0xEE;
        d.subchId = d.startAddr = d.protLevel = d.DSCTy = d.length = d.bitRate = d.FEC_scheme = d.DGflag = d.packetAddress = -7777;
        d.uepFlag = 0xEE;
        p->dataforAudioService(q, &a);       // ("fatal error, expected ..." on stderr is an answer, not a failure)
        p->dataforDataService(q, &d);
        const int av[9] = {a.subchId, a.startAddr, a.uepFlag, a.protLevel, a.length, a.bitRate, a.ASCTy, a.language, a.programType};
        const int dv[10] = {d.subchId, d.startAddr, d.uepFlag, d.protLevel, d.DSCTy, d.length, d.bitRate, d.FEC_scheme, d.DGflag,
                            d.packetAddress};
        for (int v : av) put(out, v);
        for (int v : dv) put(out, v);
    }
    std::fclose(out);
    delete p;
    return 0;
}
