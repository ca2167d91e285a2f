// Driver of tests/golden/make_rate_golden.py: one airspyHandler over a library that is not there.
// dlopen / dlsym are defined here and hand out the airspy_* functions below: the only sample rate
// is the one on the command line, airspy_start_rx keeps the handler's callback and context.  The
// int16 I/Q pairs of IN go through that callback in transfers of the given sizes (in samples, used
// in turn), and after every transfer what getSamples delivers is appended to OUT (cf32).
// usage: rate_golden RATE IN.s16 OUT.cf32 SIZE [SIZE ...]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "airspy-handler.h"

static uint32_t the_rate = 0;
static airspy_sample_block_cb_fn the_callback = nullptr;
static void *the_ctx = nullptr;
static int dummy_device;

extern "C" {
static int s_init(void) { return AIRSPY_SUCCESS; }
static int s_exit(void) { return AIRSPY_SUCCESS; }
static int s_open(struct airspy_device **d) { *d = (struct airspy_device *)&dummy_device; return AIRSPY_SUCCESS; }
static int s_close(struct airspy_device *) { return AIRSPY_SUCCESS; }
static int s_get_samplerates(struct airspy_device *, uint32_t *buffer, const uint32_t len) {
    if (len == 0) *buffer = 1;      // how many
    else buffer[0] = the_rate;
    return AIRSPY_SUCCESS;
}
static int s_set_samplerate(struct airspy_device *, uint32_t) { return AIRSPY_SUCCESS; }
static int s_start_rx(struct airspy_device *, airspy_sample_block_cb_fn cb, void *ctx) {
    the_callback = cb;
    the_ctx = ctx;
    return AIRSPY_SUCCESS;
}
static int s_stop_rx(struct airspy_device *) { return AIRSPY_SUCCESS; }
static int s_set_sample_type(struct airspy_device *, airspy_sample_type) { return AIRSPY_SUCCESS; }
static int s_set_freq(struct airspy_device *, const uint32_t) { return AIRSPY_SUCCESS; }
static int s_set_u8(struct airspy_device *, uint8_t) { return AIRSPY_SUCCESS; }
static const char *s_error_name(enum airspy_error) { return "stub"; }
static int s_board_id_read(struct airspy_device *, uint8_t *v) { *v = 0; return AIRSPY_SUCCESS; }
static const char *s_board_id_name(enum airspy_board_id) { return "stub"; }
static int s_serialno_read(struct airspy_device *, airspy_read_partid_serialno_t *r) { memset(r, 0, sizeof *r); return AIRSPY_SUCCESS; }

void *dlopen(const char *, int) { return &dummy_device; }
int dlclose(void *) { return 0; }
char *dlerror(void) { return (char *)"stub"; }
void *dlsym(void *, const char *name) {
    static const struct { const char *name; void *fn; } tab[] = {
        {"airspy_init", (void *)s_init}, {"airspy_exit", (void *)s_exit}, {"airspy_open", (void *)s_open},
        {"airspy_close", (void *)s_close}, {"airspy_get_samplerates", (void *)s_get_samplerates},
        {"airspy_set_samplerate", (void *)s_set_samplerate}, {"airspy_start_rx", (void *)s_start_rx},
        {"airspy_stop_rx", (void *)s_stop_rx}, {"airspy_set_sample_type", (void *)s_set_sample_type},
        {"airspy_set_freq", (void *)s_set_freq}, {"airspy_set_lna_gain", (void *)s_set_u8},
        {"airspy_set_mixer_gain", (void *)s_set_u8}, {"airspy_set_vga_gain", (void *)s_set_u8},
        {"airspy_set_lna_agc", (void *)s_set_u8}, {"airspy_set_mixer_agc", (void *)s_set_u8},
        {"airspy_set_rf_bias", (void *)s_set_u8}, {"airspy_error_name", (void *)s_error_name},
        {"airspy_board_id_read", (void *)s_board_id_read}, {"airspy_board_id_name", (void *)s_board_id_name},
        {"airspy_board_partid_serialno_read", (void *)s_serialno_read}};
    for (const auto &e : tab)
        if (!strcmp(e.name, name)) return e.fn;
    return nullptr;
}
}

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    the_rate = (uint32_t)strtoul(argv[1], nullptr, 10);
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    fseek(in, 0, SEEK_END);
    std::vector<int16_t> x((size_t)ftell(in) / sizeof(int16_t));
    fseek(in, 0, SEEK_SET);
    if (fread(x.data(), sizeof(int16_t), x.size(), in) != x.size()) return 3;
    QSettings settings;
    bool ok = false;
    airspyHandler h(&settings, &ok);
    if (!ok || !h.restartReader() || !the_callback) return 4;
    std::vector<DSPCOMPLEX> got(256 * 1024);
    const size_t n = x.size() / 2;
    for (size_t at = 0, turn = 0; at < n; turn++) {
        size_t size = strtoul(argv[4 + turn % (argc - 4)], nullptr, 10);
        if (size > n - at) size = n - at;
        std::vector<int16_t> piece(x.begin() + 2 * at, x.begin() + 2 * (at + size));   // a block of exactly its length
        airspy_transfer t;
        memset(&t, 0, sizeof t);
        t.ctx = the_ctx;
        t.samples = piece.data();
        t.sample_count = (int)size;
        t.sample_type = AIRSPY_SAMPLE_INT16_IQ;
        if (the_callback(&t) != 0) return 5;
        const int32_t m = h.getSamples(got.data(), (int32_t)got.size());
        fwrite(got.data(), sizeof(DSPCOMPLEX), (size_t)m, out);
        at += size;
    }
    fclose(out);
    return 0;
}
