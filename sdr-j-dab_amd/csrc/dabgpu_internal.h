// dabgpu_internal.h -- what the two host translation units of the C ABI share:
// dabgpu_ctx.cpp (errors, host tables, context, operators) and dabgpu_pipe.cpp (streaming pipeline).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "../../include/dabgpu.h"
#include "dab_kernels.h"

struct dabgpu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[16] = {};
    float2 *osc = nullptr, *ref = nullptr;
    double2 *nco = nullptr;
    uint32_t *prbs = nullptr;
    float2 *w2048 = nullptr;
    int16_t *carrier_bin = nullptr;
    float *refarg = nullptr;
    uint8_t *dptab = nullptr;    // DAB+ tables (HostTables::dptab)
    uint8_t *fic_inv = nullptr;  // the FIC profile's inverse depuncturing table (make_inv)
    int32_t *err = nullptr;      // device error word (KERR_* bits)
    int32_t *h_err = nullptr;    // its pinned host copy (read after every synchronising pass)
    dab::OfdmTables T{};
    // growable scratch
    void *scratch[8] = {};
    size_t scratch_sz[8] = {};
};

namespace dab {

// sets dabgpu_last_error's text (per thread), returns code
int fail(int code, const char *fmt, ...);
#define HIPCHK(expr)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(DABGPU_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                                      \
    } while (0)

enum { SC_DEC = 0, SC_PROF = 1, SC_I32 = 2, SC_FRAMES = 3, SC_FC = 4, SC_MISC = 5, SC_ACQ = 6 };
int scratch(dabgpu_ctx *c, int slot, size_t bytes, void **p);
// read (and clear) the device error word; call after a stream synchronisation
int kernel_errors(dabgpu_ctx *c);

constexpr int kMaxChunks = 25;
// k_demod workgroups per frame; extra: FFTs every chunk adds besides its warm-up symbol
int demod_chunks(int n, int extra = 0);

int make_profile(const dabgpu_subch &s, Profile &p);     // deconvolve.cpp:142-366; nonzero: undefined
Profile fic_profile();                                   // fic-handler.cpp:254-288
std::vector<uint8_t> make_inv(const Profile &P);         // inverse depuncturing table

}  // namespace dab
