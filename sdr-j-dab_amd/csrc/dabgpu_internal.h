// dabgpu_internal.h -- what the host translation units of the C ABI share: dabgpu_ctx.cpp (errors,
// host tables, context, operators) and the streaming pipeline's two, dabgpu_pipe.cpp and
// dabgpu_layers.cpp (which share the pipeline's own state through dabgpu_pipe.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <algorithm>
#include <map>
#include <utility>
#include <vector>
#include "../../include/dabgpu.h"
#include "dab_kernels.h"

namespace dab {

// The GPU resources the context and the pipeline hold, each owned by a move-only handle that
// releases it in its destructor.  Their calls return the runtime's status (for HIPCHK).
template <class T>
struct DevBuf {                                          // device memory: n elements of T
    T *ptr = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept { swap(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { swap(o); return *this; }   // (the old memory goes with o)
    ~DevBuf() { reset(); }
    void swap(DevBuf &o) { std::swap(ptr, o.ptr); std::swap(n, o.n); }
    void reset() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        n = 0;
    }
    // at least 256 bytes: an empty table is still a valid pointer
    hipError_t alloc(size_t count) {
        reset();
        const hipError_t e = hipMalloc((void **)&ptr, std::max<size_t>(count * sizeof(T), 256));
        if (e == hipSuccess) n = count;
        else ptr = nullptr;
        return e;
    }
    hipError_t zalloc(size_t count) {                    // allocate, all bytes zero
        const hipError_t e = alloc(count);
        return e != hipSuccess ? e : hipMemset(ptr, 0, count * sizeof(T));
    }
    hipError_t put(const std::vector<T> &v) {            // allocate and upload
        const hipError_t e = alloc(v.size());
        return e != hipSuccess ? e : hipMemcpy(ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    operator T *() const { return ptr; }
};

template <class T>
struct PinBuf {                                          // pinned host memory
    T *ptr = nullptr;
    PinBuf() = default;
    PinBuf(PinBuf &&o) noexcept { std::swap(ptr, o.ptr); }
    PinBuf &operator=(PinBuf &&o) noexcept { std::swap(ptr, o.ptr); return *this; }
    ~PinBuf() { reset(); }
    void reset() {
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr;
    }
    hipError_t alloc(size_t count) {
        reset();
        const hipError_t e = hipHostMalloc((void **)&ptr, count * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) ptr = nullptr;
        return e;
    }
    operator T *() const { return ptr; }
};

// An event that knows whether it was ever recorded: waiting for one that was not is a no-op
struct Event {
    hipEvent_t e = nullptr;
    bool rec = false;
    Event() = default;
    Event(Event &&o) noexcept { swap(o); }
    Event &operator=(Event &&o) noexcept { swap(o); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    void swap(Event &o) { std::swap(e, o.e); std::swap(rec, o.rec); }
    hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&e, flags); }
    hipError_t record(hipStream_t s) {
        const hipError_t r = hipEventRecord(e, s);
        if (r == hipSuccess) rec = true;
        return r;
    }
    hipError_t wait_on(hipStream_t s) const { return rec ? hipStreamWaitEvent(s, e, 0) : hipSuccess; }
    hipError_t sync() const { return rec ? hipEventSynchronize(e) : hipSuccess; }
    hipError_t query() const { return rec ? hipEventQuery(e) : hipSuccess; }   // hipSuccess: ready
    bool recorded() const { return rec; }
};

// A non-blocking stream; its destructor waits for it before destroying it
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept { std::swap(s, o.s); }
    Stream &operator=(Stream &&o) noexcept { std::swap(s, o.s); return *this; }
    ~Stream() {
        if (!s) return;
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    hipError_t create(int priority) { return hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority); }
    hipError_t sync() const { return s ? hipStreamSynchronize(s) : hipSuccess; }
    operator hipStream_t() const { return s; }
};

// airspyHandler's tables for one input rate, on the device and (mapTable_int) on the host: the
// samples a piece of consecutive outputs reads decide k_rate_convert's passes
struct RateEntry {
    DevBuf<RateTab> tab;
    std::vector<int16_t> base;      // [2048]
};

}  // namespace dab

// Members are destroyed in reverse order of declaration: the stream comes last, so it has
// drained and gone before the memory its kernels used is freed.
struct dabgpu_ctx {
    int device = 0;
    dab::Event ev[16];
    dab::DevBuf<float2> osc, ref;
    dab::DevBuf<double2> nco;
    dab::DevBuf<uint32_t> prbs;
    dab::DevBuf<float2> w2048;
    dab::DevBuf<int16_t> carrier_bin;
    dab::DevBuf<float> refarg;
    dab::DevBuf<uint8_t> dptab;    // DAB+ tables (HostTables::dptab)
    dab::DevBuf<uint8_t> fic_inv;  // the FIC profile's inverse depuncturing table (make_inv)
    dab::DevBuf<uint8_t> mp2tab;   // layer II tables (Mp2Tabs, mp2_host_tables)
    dab::DevBuf<float> audiotab;   // audioSink's filter kernels (audio_host_fir)
    std::map<int, dab::RateEntry> ratetab;   // rate conversion tables by input rate, each made at the rate's first use
    dab::DevBuf<int32_t> err;      // device error word (KERR_* bits)
    dab::PinBuf<int32_t> h_err;    // its pinned host copy (read after every synchronising pass)
    dab::OfdmTables T{};
    dab::DevBuf<uint8_t> scratch[10];   // growable scratch (dab::scratch)
    dab::Stream stream;
    ~dabgpu_ctx() {
        (void)hipSetDevice(device);
        (void)stream.sync();
    }
};

namespace dab {

// sets dabgpu_last_error's text (per thread), returns code
int fail(int code, const char *fmt, ...);
// (a failed allocation reports DABGPU_E_NOMEM, every other runtime error DABGPU_E_HIP)
#define HIPCHK(expr)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? DABGPU_E_NOMEM : DABGPU_E_HIP, "%s: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                \
    } while (0)

enum { SC_DEC = 0, SC_PROF = 1, SC_I32 = 2, SC_FRAMES = 3, SC_FC = 4, SC_MISC = 5, SC_ACQ = 6, SC_MP2 = 7, SC_MOT = 8,
       SC_AUDIO = 9 };
int scratch(dabgpu_ctx *c, int slot, size_t bytes, void **p);
// read (and clear) the device error word; call after a stream synchronisation
int kernel_errors(dabgpu_ctx *c);
// DABGPU_E_BOUNDS with the text for a nonzero error word (KERR_* bits)
int bounds_error(int32_t e);

constexpr int kMaxChunks = 25;
// k_demod workgroups per frame; extra: FFTs every chunk adds besides its warm-up symbol
int demod_chunks(int n, int extra = 0);

int make_profile(const dabgpu_subch &s, Profile &p);     // deconvolve.cpp:142-366; nonzero: undefined
Profile fic_profile();                                   // fic-handler.cpp:254-288
std::vector<uint8_t> make_inv(const Profile &P);         // inverse depuncturing table
std::vector<uint8_t> mp2_host_tables();                  // an Mp2Tabs (k_mp2.hip)
int mp2_tables(dabgpu_ctx *c, const Mp2Tabs **out);      // the context's device copy, made at first use
const std::vector<float> &audio_host_fir();              // DABGPU_TABLE_AUDIO_FIR, float[3][5]
int audio_tables(dabgpu_ctx *c, const float **out);      // the context's device copy, made at first use
int rate_tables(dabgpu_ctx *c, int rate, const RateEntry **out);   // the context's entry for a rate, made at first use

}  // namespace dab
