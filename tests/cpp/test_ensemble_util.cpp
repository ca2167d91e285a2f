// TEST INFRASTRUCTURE: the pure pieces of ensembleDecoder (sdr-j-dab_amd/host/ensemble_util.h), built
// from the header alone with its own main (tests/test_ensemble_util_cpu.py): entries_flagged and
// count_flagged against the per-layer loops they replaced, restated here; unpack_bits at lengths that
// are no multiple of 8; wanted_flags against the two spellings it replaced; sdr_payload on files this
// program writes.  Prints "ENSEMBLE UTIL OK" when everything held.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>
#include "ensemble_util.h"

using namespace dabgpu;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("MISMATCH: " __VA_ARGS__); std::printf("\n"); fails++; } } while (0)

struct err : std::runtime_error {
    int code;
    err(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

// ---- the loops of the decoder's step() before entries_flagged, as they stood ------------------
static std::vector<int> one_flag(const std::vector<dabgpu_subch> &t, int flag) {       // DAB+, MP2, audio, packet, IP's packet slots
    std::vector<int> slot;
    for (int k = 0; k < (int)t.size(); k++)
        if (t[k].flags & flag) slot.push_back(k);
    return slot;
}
static std::vector<int> two_flags(const std::vector<dabgpu_subch> &t, int a, int b) {   // PAD (DAB+ and PAD), MOT (packet and MOT)
    std::vector<int> slot;
    for (int k = 0; k < (int)t.size(); k++)
        if ((t[k].flags & a) && (t[k].flags & b)) slot.push_back(k);
    return slot;
}
// (the loops that used the lists ran `j < (int)slot.size() && j < n`)
static std::vector<int> capped(std::vector<int> slot, int n) {
    if ((int)slot.size() > n) slot.resize((size_t)std::max(0, n));
    return slot;
}

static void test_slots() {
    std::mt19937 rng(20240607);
    const int all = DABGPU_SUBCH_DABPLUS | DABGPU_SUBCH_MP2 | DABGPU_SUBCH_PACKET | DABGPU_SUBCH_MOT | DABGPU_SUBCH_PAD | DABGPU_SUBCH_IP |
                    DABGPU_SUBCH_AUDIO;
    long lists = 0;
    for (int round = 0; round < 400; round++) {
        std::vector<dabgpu_subch> t(rng() % 65);
        const int sparse = round % 3;                // dense flags, few flags, none or all
        for (dabgpu_subch &e : t) {
            e = dabgpu_subch{(int16_t)(rng() % 864), (int16_t)(rng() % 200), (int16_t)(8 * (1 + rng() % 16)), 0, 1, 0};
            e.flags = sparse == 0 ? (int)(rng() & all) : sparse == 1 ? (int)(rng() & rng() & rng() & all) : (rng() & 1 ? all : 0);
        }
        struct { int mask; std::vector<int> want; } cases[] = {
            {DABGPU_SUBCH_DABPLUS, one_flag(t, DABGPU_SUBCH_DABPLUS)},
            {DABGPU_SUBCH_DABPLUS | DABGPU_SUBCH_PAD, two_flags(t, DABGPU_SUBCH_DABPLUS, DABGPU_SUBCH_PAD)},
            {DABGPU_SUBCH_MP2, one_flag(t, DABGPU_SUBCH_MP2)},
            {DABGPU_SUBCH_AUDIO, one_flag(t, DABGPU_SUBCH_AUDIO)},
            {DABGPU_SUBCH_PACKET, one_flag(t, DABGPU_SUBCH_PACKET)},
            {DABGPU_SUBCH_PACKET | DABGPU_SUBCH_MOT, two_flags(t, DABGPU_SUBCH_PACKET, DABGPU_SUBCH_MOT)},
            {DABGPU_SUBCH_PACKET, one_flag(t, DABGPU_SUBCH_PACKET)},                     // the IP block's list
        };
        for (const auto &c : cases) {
            const int n = (int)c.want.size();
            for (int cap : {0, 1, n / 2, n, n + 1, 64, 1000}) {
                CHECK(entries_flagged(t, c.mask, cap) == capped(c.want, cap), "round %d mask %d cap %d: entries_flagged", round, c.mask, cap);
                lists++;
            }
            CHECK(count_flagged(t, c.mask) == n, "round %d mask %d: count_flagged %d for %d", round, c.mask, count_flagged(t, c.mask), n);
        }
        // the constructor's and the IP block's counts test one flag, or both of two
        for (int f : {DABGPU_SUBCH_DABPLUS, DABGPU_SUBCH_MP2, DABGPU_SUBCH_AUDIO, DABGPU_SUBCH_PACKET, DABGPU_SUBCH_MOT, DABGPU_SUBCH_PAD}) {
            int n = 0;
            for (const dabgpu_subch &sc : t)
                if (sc.flags & f) n++;
            CHECK(count_flagged(t, f) == n, "round %d flag %d: count_flagged", round, f);
        }
        bool any_ip = false;
        for (const dabgpu_subch &e : t) any_ip |= (e.flags & DABGPU_SUBCH_PACKET) && (e.flags & DABGPU_SUBCH_IP);
        CHECK((count_flagged(t, DABGPU_SUBCH_PACKET | DABGPU_SUBCH_IP) > 0) == any_ip, "round %d: any IP entry", round);
    }
    std::printf("slots: %ld lists\n", lists);
}

static void test_unpack() {
    std::mt19937 rng(7);
    for (int nbits : {0, 1, 7, 8, 9, 13, 255, 256, 257, 768, 24 * 8 + 3, 3071}) {
        std::vector<uint8_t> packed((size_t)(nbits + 7) / 8 + 1), out((size_t)nbits + 2, 0xAA);
        for (uint8_t &b : packed) b = (uint8_t)rng();
        unpack_bits(packed.data(), nbits, out.data() + 1);
        CHECK(out[0] == 0xAA && out[(size_t)nbits + 1] == 0xAA, "unpack_bits %d: wrote outside", nbits);
        for (int i = 0; i < nbits; i++)
            CHECK(out[(size_t)i + 1] == ((packed[(size_t)i / 8] >> (7 - i % 8)) & 1), "unpack_bits %d: bit %d", nbits, i);
    }
}

// the mask of step()'s dabgpu_pipe_fic call and the five booleans of its fib_processor::subchannels call, as they stood
static void test_wanted() {
    for (int cb = 0; cb < 64; cb++)
        for (int n = 0; n < 32; n++) {
            const bool pcm = cb & 1, audio = cb & 2, dg = cb & 4, mot = cb & 8, ip = cb & 16, pad = cb & 32;
            const int nmp = n & 1, naudio = (n >> 1) & 1, npk = 2 * ((n >> 2) & 1), nmot = (n >> 3) & 1, npad = 3 * ((n >> 4) & 1);
            const int mask = ((pcm || (audio && naudio > 0)) && nmp > 0 ? DABGPU_SUBCH_MP2 : 0) | (dg && npk > 0 ? DABGPU_SUBCH_PACKET : 0) |
                             (mot && nmot > 0 ? DABGPU_SUBCH_MOT : 0) | (ip && npk > 0 ? DABGPU_SUBCH_IP : 0) | (pad && npad > 0 ? DABGPU_SUBCH_PAD : 0);
            const bool b_mp2 = (pcm || (audio && naudio > 0)) && nmp > 0, b_packet = dg && npk > 0, b_mot = mot && nmot > 0,
                       b_pad = pad && npad > 0, b_ip = ip && npk > 0;
            const int w = wanted_flags({pcm, audio, dg, mot, ip, pad, nmp, naudio, npk, nmot, npad});
            CHECK(w == mask, "wanted_flags callbacks %d slots %d: %d for %d", cb, n, w, mask);
            CHECK(((w & DABGPU_SUBCH_MP2) != 0) == b_mp2 && ((w & DABGPU_SUBCH_PACKET) != 0) == b_packet && ((w & DABGPU_SUBCH_MOT) != 0) == b_mot &&
                      ((w & DABGPU_SUBCH_PAD) != 0) == b_pad && ((w & DABGPU_SUBCH_IP) != 0) == b_ip,
                  "wanted_flags callbacks %d slots %d: the host parse's booleans", cb, n);
        }
}

// ---- sdr_payload ---------------------------------------------------------------------------
typedef std::vector<uint8_t> blob;
static void put(blob &b, const char *s) { b.insert(b.end(), s, s + 4); }
static void u16(blob &b, unsigned v) { b.push_back((uint8_t)v); b.push_back((uint8_t)(v >> 8)); }
static void u32(blob &b, unsigned v) { u16(b, v & 0xFFFF); u16(b, v >> 16); }
static void fmt16(blob &b, unsigned tag, unsigned channels, unsigned rate, unsigned bits) {
    u16(b, tag); u16(b, channels); u32(b, rate); u32(b, rate * channels * bits / 8); u16(b, channels * bits / 8); u16(b, bits);
}
static blob riff() { blob b; put(b, "RIFF"); u32(b, 0); put(b, "WAVE"); return b; }
static void data(blob &b, unsigned n) { put(b, "data"); u32(b, n); b.insert(b.end(), n, 0x5A); }

// the offset and size sdr_payload gives for the file, or "error: <what>"
static std::string payload_of(const std::string &dir, const char *name, const blob &b, int64_t *off, int64_t *n) {
    const std::string path = dir + "/" + name;
    std::FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(b.data(), 1, b.size(), f) != b.size()) std::abort();
    std::fclose(f);
    f = std::fopen(path.c_str(), "rb");
    std::string r = "ok";
    try {
        const std::pair<int64_t, int64_t> p = sdr_payload<err>(f, path);
        *off = p.first;
        *n = p.second;
    } catch (const err &e) {
        r = std::string("error: ") + e.what();
        if (e.code != DABGPU_E_ARG) r += " (not DABGPU_E_ARG)";
    }
    std::fclose(f);
    std::remove(path.c_str());
    return r;
}

static void test_sdr(const std::string &dir) {
    int64_t off = 0, n = 0;
    std::string r;
    {   // a plain PCM16 header: RIFF(12) + fmt(8 + 16) + data header(8)
        blob b = riff(); put(b, "fmt "); u32(b, 16); fmt16(b, 1, 2, 2048000, 16); data(b, 4000);
        r = payload_of(dir, "plain.sdr", b, &off, &n);
        CHECK(r == "ok" && off == 44 && n == 4000, "plain PCM16: %s offset %lld size %lld", r.c_str(), (long long)off, (long long)n);
    }
    {   // WAVE_FORMAT_EXTENSIBLE: 40 bytes of fmt, the subformat's first two bytes at 24
        blob b = riff(); put(b, "fmt "); u32(b, 40); fmt16(b, 0xFFFE, 2, 2048000, 16); u16(b, 22); u16(b, 16); u32(b, 3); u16(b, 1);
        b.insert(b.end(), 14, 0); data(b, 1024);
        r = payload_of(dir, "ext.sdr", b, &off, &n);
        CHECK(r == "ok" && off == 68 && n == 1024, "extensible: %s offset %lld size %lld", r.c_str(), (long long)off, (long long)n);
        b[12 + 8 + 24] = 3;                          // the subformat says IEEE float
        r = payload_of(dir, "extf.sdr", b, &off, &n);
        CHECK(r.find("not a recorded DAB file") != std::string::npos, "extensible float: %s", r.c_str());
    }
    {   // an odd-sized chunk (7 bytes + its pad byte) before fmt
        blob b = riff(); put(b, "LIST"); u32(b, 7); b.insert(b.end(), 8, 'x'); put(b, "fmt "); u32(b, 16); fmt16(b, 1, 2, 2048000, 16); data(b, 10);
        r = payload_of(dir, "odd.sdr", b, &off, &n);
        CHECK(r == "ok" && off == 44 + 16 && n == 10, "odd chunk: %s offset %lld size %lld", r.c_str(), (long long)off, (long long)n);
    }
    {   // no data chunk
        blob b = riff(); put(b, "fmt "); u32(b, 16); fmt16(b, 1, 2, 2048000, 16);
        r = payload_of(dir, "nodata.sdr", b, &off, &n);
        CHECK(r.find("no data chunk") != std::string::npos, "missing data chunk: %s", r.c_str());
    }
    {   // a wrong rate
        blob b = riff(); put(b, "fmt "); u32(b, 16); fmt16(b, 1, 2, 2000000, 16); data(b, 16);
        r = payload_of(dir, "rate.sdr", b, &off, &n);
        CHECK(r.find("not a recorded DAB file") != std::string::npos, "wrong rate: %s", r.c_str());
    }
    {   // cut inside fmt
        blob b = riff(); put(b, "fmt "); u32(b, 16); fmt16(b, 1, 2, 2048000, 16); b.resize(b.size() - 6);
        r = payload_of(dir, "cut.sdr", b, &off, &n);
        CHECK(r.find("bad fmt chunk") != std::string::npos, "cut inside fmt: %s", r.c_str());
    }
    {   // not RIFF at all
        blob b(64, 0);
        r = payload_of(dir, "zero.sdr", b, &off, &n);
        CHECK(r.find("not a RIFF/WAVE file") != std::string::npos, "no RIFF header: %s", r.c_str());
    }
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;                         // a directory to write the .sdr files into
    test_slots();
    test_unpack();
    test_wanted();
    test_sdr(argv[1]);
    if (fails) {
        std::printf("FAILED: %d mismatches\n", fails);
        return 1;
    }
    std::printf("ENSEMBLE UTIL OK\n");
    return 0;
}
