// Input rate conversion: a stream sampled at 1000 M Hz -> 2.048 MHz cf32, the linear interpolation
// of airspyHandler::data_available (airspy-handler.cpp:333-359), bit for bit what
// host/rate_converter.h's rateConverter does.
//
// Block b of a stream reads inputs x[M b .. M b + M] and writes outputs 2048 b + j:
//   out = x[k + 1] * r + x[k] * (1.0f - r),   k = M b + base[j], r = frac[j]   (re and im alike)
// with every product, the 1.0f - r and the sum rounded to fp32 on its own (the Makefile builds this
// file with -ffp-contract=off: the default would fuse them).  base / frac are the handler's
// mapTable_int / mapTable_float, built on the host and kept per rate by the context.
//
//   k_rate_convert<FORMAT, outputs per lane and piece>   one workgroup per (block, stream), grid = largest block count x streams;
//                  a workgroup past its stream's block count exits at once.  It stages its input
//                  samples in LDS as the stream holds them (2, 4 or 8 bytes a sample), 16 bytes per
//                  lane and load, and converts them to float as it reads them back: lane t does
//                  outputs t, t + 256, ..., one float2 store each, consecutive lanes to consecutive
//                  addresses.  The LDS image is RATE_LDS_BYTES at every rate and format, so eight
//                  workgroups (all 32 wave slots) fit a CU: a block whose M + 1 samples are more is
//                  done in 2, 4 or 8 pieces of consecutive outputs, each staging only its own span.
// A block starts wherever sample M b lies: on a 4-byte boundary for int16 pairs with M b odd, on
// a 2-byte one for u8.  The 16-byte loads are declared with the sample's alignment (the target
// reads them unaligned); the last, partial 16 bytes of a span are loaded sample by sample, so
// nothing outside x[M b .. M b + M] is ever read.
#include <algorithm>
#include "dab_device.h"
#include "dab_kernels.h"

namespace dab {

// a sample as the stream holds it, and as the float pair the interpolation reads
template <int FMT> struct RateFmt {
    typedef typename IqFmt<FMT>::raw raw;
    static constexpr int bps = IqFmt<FMT>::bps;
    __device__ static float2 cvt(raw v) { return IqFmt<FMT>::cvt(v); }
};
template <> struct RateFmt<DABGPU_IQ_S12> {          // x / 2048 (airspy-handler.cpp:340-341): exact
    typedef uint32_t raw;
    static constexpr int bps = 4;
    __device__ static float2 cvt(raw v) {
        const float2 s = IqFmt<DABGPU_IQ_S16>::scaled(v);
        return make_float2(s.x * 0x1p-11f, s.y * 0x1p-11f);
    }
};
template <int BPS> struct RateElem;                  // what LDS holds per sample
template <> struct RateElem<2> { typedef uint16_t type; };
template <> struct RateElem<4> { typedef uint32_t type; };
template <> struct RateElem<8> { typedef float2 type; };

// 16 bytes at g + 16 c, g aligned to a sample of BPS bytes only
template <int BPS>
__device__ __forceinline__ uint4 rate_load16(const char *g, int c) {
    uint4 v;
    __builtin_memcpy(&v, __builtin_assume_aligned(g + 16 * c, BPS < 4 ? BPS : 4), 16);
    return v;
}

// NIT: outputs per lane and piece, 8 / passes
template <int FMT, int NIT>
__global__ __launch_bounds__(256) void k_rate_convert(RateJob J) {
    typedef RateFmt<FMT> F;
    typedef typename RateElem<F::bps>::type elem;
    constexpr int PER16 = 16 / F::bps;               // samples per 16-byte load
    constexpr int S = 256 * NIT;                     // outputs per piece
    __shared__ uint4 lds[RATE_LDS_BYTES / 16];
    const int t = threadIdx.x;
    const int64_t s = blockIdx.y, b = blockIdx.x;
    if (b >= J.blocks[s]) return;                    // past the stream's own blocks
    const char *x = (const char *)J.src + (J.src_stride * s + b * J.M) * F::bps;
    float2 *o = (float2 *)J.out + (J.out_stride * s + 2048 * b);
    const elem *sm = (const elem *)lds;
    bool bad = false;
    for (int p = 0; p < 8 / NIT; p++) {
        // the piece's outputs j0 .. j0 + S - 1 read samples k0 .. k1 of the block (the tables ascend)
        const int j0 = p * S, k0 = J.first[p], k1 = J.last[p], n = k1 - k0 + 1;
        if (k0 < 0 || k1 > J.M || n < 2 || n * F::bps > RATE_LDS_BYTES) {
            if (t == 0) atomicOr(J.err, KERR_RATE);
            return;
        }
        int k[NIT];
        float r[NIT];
#pragma unroll
        for (int i = 0; i < NIT; i++) {
            k[i] = J.tab->base[j0 + 256 * i + t] - k0;
            r[i] = J.tab->frac[j0 + 256 * i + t];
        }
        if (p) __syncthreads();                      // the piece before is read
        const char *g = x + (int64_t)k0 * F::bps;
        const int full = n / PER16;
        // up to four 16-byte loads in flight per lane: a lane past the end repeats the last one and stores nothing
        for (int c0 = 0; c0 < full; c0 += 1024) {
            const int c = c0 + t;
            const uint4 v0 = rate_load16<F::bps>(g, min(c, full - 1));
            uint4 v1 = make_uint4(0, 0, 0, 0), v2 = v1, v3 = v1;
            if (c0 + 256 < full) v1 = rate_load16<F::bps>(g, min(c + 256, full - 1));
            if (c0 + 512 < full) v2 = rate_load16<F::bps>(g, min(c + 512, full - 1));
            if (c0 + 768 < full) v3 = rate_load16<F::bps>(g, min(c + 768, full - 1));
            if (c < full) lds[c] = v0;
            if (c + 256 < full) lds[c + 256] = v1;
            if (c + 512 < full) lds[c + 512] = v2;
            if (c + 768 < full) lds[c + 768] = v3;
        }
        if (t < n - full * PER16) ((elem *)lds)[full * PER16 + t] = ((const elem *)g)[full * PER16 + t];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NIT; i++) {
            const bool in = k[i] >= 0 && k[i] + 1 < n;
            bad = bad || !in;
            const int kk = in ? k[i] : 0;
            const float q = 1.0f - r[i];
            const float2 a = F::cvt((typename F::raw)sm[kk + 1]), c = F::cvt((typename F::raw)sm[kk]);
            if (in) o[j0 + 256 * i + t] = make_float2(a.x * r[i] + c.x * q, a.y * r[i] + c.y * q);
        }
    }
    if (bad) atomicOr(J.err, KERR_RATE);
}

template <int FMT>
static hipError_t rate_launch(hipStream_t st, dim3 grid, const RateJob &J) {
    switch (J.passes) {
    case 1: hipLaunchKernelGGL((k_rate_convert<FMT, 8>), grid, dim3(256), 0, st, J); break;
    case 2: hipLaunchKernelGGL((k_rate_convert<FMT, 4>), grid, dim3(256), 0, st, J); break;
    case 4: hipLaunchKernelGGL((k_rate_convert<FMT, 2>), grid, dim3(256), 0, st, J); break;
    case 8: hipLaunchKernelGGL((k_rate_convert<FMT, 1>), grid, dim3(256), 0, st, J); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_rate_convert(hipStream_t st, int format, const RateJob &J) {
    if (J.n_streams < 0 || J.n_streams > RATE_GROUP) return hipErrorInvalidValue;
    int32_t most = 0;
    for (int s = 0; s < J.n_streams; s++) most = std::max(most, J.blocks[s]);
    if (most <= 0) return hipSuccess;
    const dim3 grid((unsigned)most, (unsigned)J.n_streams);
    switch (format) {
    case DABGPU_IQ_F32: return rate_launch<DABGPU_IQ_F32>(st, grid, J);
    case DABGPU_IQ_U8: return rate_launch<DABGPU_IQ_U8>(st, grid, J);
    case DABGPU_IQ_S16: return rate_launch<DABGPU_IQ_S16>(st, grid, J);
    case DABGPU_IQ_S12: return rate_launch<DABGPU_IQ_S12>(st, grid, J);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace dab
