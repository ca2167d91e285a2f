// Audio output layer: int16 PCM at the frame's own rate -> audioSink's 48 kHz float stereo signal.
// audioSink::audioOut and its four bodies (audiosink.cpp:235-360) over LowPassFIR::Pass
// (fir-filters.cpp:78-92), bit for bit what host/msc_consumers.cpp's audioResampler does.
//
// A sample is (float)V / 32767 (fp32 division, correctly rounded: equal to the reference's double
// division rounded to float for every int16).  16000, 24000 and 32000 Hz go through a 5-tap FIR
// over the zero-stuffed input, so an output pair depends on the current input pair and at most
// the two before it: with s[n] the stuffed sequence, out[n] = sum_{i=0..4} s[n-i] * k[i], summed in
// the order i = 0..4 from +0, every product and sum rounded to fp32 on its own (the Makefile builds
// this file with -ffp-contract=off: the default would fuse them).  Two things of the reference's
// complex arithmetic are left out because no bit depends on them: the terms of stuffed zeros, and
// the "- s.im * 0" / "s.re * 0 +" halves of each complex product.  Each is a zero of either sign; the accumulator starts at +0, +0 plus a zero is
// +0 and a nonzero sum stays what it is, so the accumulator is never -0 and adding a zero of either
// sign never changes it.
//
//   k_audio_out    one workgroup per (chain, call), lanes over output pairs: a dword load per input
//                  pair, one float2 store per output pair, consecutive lanes to consecutive
//                  addresses.  The workgroup finds its filter's history by walking back over the
//                  chain's calls of this launch to the last ones of its rate, then to the carried
//                  state; it reads the state and never writes it.
//   k_audio_state  behind it, one lane per (chain, filter): the filter's last two input pairs
//                  after the launch's calls, by the same walk from the chain's end, in place.
// No LDS, no cross-lane traffic, nothing atomic.  A call whose rate and amount would leave its
// input or output row (info records are the caller's memory) is no call, in both kernels alike.
#include "dab_device.h"
#include "dab_kernels.h"

namespace dab {

struct AudioCall {
    int f;        // 0 / 1 / 2: through the 16000 / 24000 / 32000 filter; -1: scaled only
    int amount;   // input pairs
    int n_out;    // output pairs, 0: no call
};

__device__ __forceinline__ AudioCall audio_call(const AudioJob &J, int c, int64_t row0, int j) {
    int rate, amount;
    if (J.info) {
        const dabgpu_mp2_info *r = J.info + row0 + j * J.in_c;
        rate = r->status == 2 ? r->sample_rate : 0;
        amount = J.fixed_amount;
    } else {
        rate = J.rates[(int64_t)c * J.chain_len + j];
        amount = J.amounts[(int64_t)c * J.chain_len + j];
    }
    AudioCall k{-1, 0, 0};
    if (rate == 0 || amount <= 0 || amount > J.in_pairs) return k;
    k.f = rate == 16000 ? 0 : rate == 24000 ? 1 : rate == 32000 ? 2 : -1;
    const int64_t n = k.f < 0 ? amount : k.f == 1 ? 2 * (int64_t)amount : k.f == 0 ? 3 * (int64_t)amount : 3 * (int64_t)amount / 2;
    if (n > J.out_pairs || (k.f == 2 && (amount & 1))) return k;
    k.amount = amount;
    k.n_out = (int)n;
    return k;
}

// call j's input pairs, one dword each (left | right << 16)
__device__ __forceinline__ const uint32_t *audio_pcm(const AudioJob &J, int64_t row0, int j) {
    return (const uint32_t *)J.pcm + (row0 + j * J.in_c) * J.in_pairs;
}

// the chain's input rows start at row0; false: the chain has no calls (its source slot is absent)
__device__ __forceinline__ bool audio_chain(const AudioJob &J, int c, int64_t &row0) {
    const int64_t s = c / J.cdiv;
    row0 = s * J.in_a;
    if (!J.src) return true;
    const int v = J.src[c];
    row0 += v - s * J.in_c;
    return v >= 0;
}

// The last pair (h1) and the one before it (h2) that filter f of chain c saw before its call j:
// from the calls before it in this launch, newest first, then from the carried state
__device__ __forceinline__ void audio_history(const AudioJob &J, int c, int64_t row0, int j, int f, int need, uint32_t &h1,
                                              uint32_t &h2) {
    int got = 0;
    h1 = h2 = 0;
    for (int jj = j - 1; jj >= 0 && got < need; jj--) {
        const AudioCall q = audio_call(J, c, row0, jj);
        if (!q.n_out || q.f != f) continue;
        const uint32_t *y = audio_pcm(J, row0, jj);
        for (int i = q.amount - 1; i >= 0 && got < need; i--, got++) {
            const uint32_t v = y[i];
            if (got == 0) h1 = v;
            else h2 = v;
        }
    }
    if (got < need) {
        const uint32_t *S = J.state[c].hist[f];
        if (got == 0) {
            h1 = S[0];
            h2 = S[1];
        } else {
            h2 = S[0];
        }
    }
}

__device__ __forceinline__ float2 audio_scale(uint32_t v) {
    return make_float2(__fdiv_rn((float)(int16_t)(v & 0xFFFFu), 32767.0f), __fdiv_rn((float)(int16_t)(v >> 16), 32767.0f));
}
// acc + x * k, both channels
__device__ __forceinline__ float2 audio_mac(float2 acc, float2 x, float k) {
    return make_float2(__fadd_rn(acc.x, __fmul_rn(x.x, k)), __fadd_rn(acc.y, __fmul_rn(x.y, k)));
}

// Output pairs of one call through a filter: Pass result n = STEP * p of the call, input pair
// m = n / UP at phase ph = n % UP, taps ph, ph + UP, ph + 2 UP (< 5) on input pairs m, m-1, m-2
template <int UP, int STEP>
__device__ __forceinline__ void audio_filter(const uint32_t *x, float2 *o, int n_out, uint32_t h1, uint32_t h2, const float *k) {
    const float k0 = k[0], k1 = k[1], k2 = k[2], k3 = k[3], k4 = k[4];
    for (int p = threadIdx.x; p < n_out; p += blockDim.x) {
        const int n = STEP * p, m = n / UP, ph = n - m * UP;
        const float2 x0 = audio_scale(x[m]);
        const float2 x1 = audio_scale(m >= 1 ? x[m - 1] : h1);
        float2 acc = make_float2(0.0f, 0.0f);
        if (UP == 2) {
            acc = audio_mac(acc, x0, ph ? k1 : k0);
            acc = audio_mac(acc, x1, ph ? k3 : k2);
            if (!ph) acc = audio_mac(acc, audio_scale(m >= 2 ? x[m - 2] : m == 1 ? h1 : h2), k4);
        } else {
            acc = audio_mac(acc, x0, ph == 0 ? k0 : ph == 1 ? k1 : k2);
            if (ph < 2) acc = audio_mac(acc, x1, ph ? k4 : k3);
        }
        o[p] = acc;
    }
}

__global__ __launch_bounds__(256) void k_audio_out(AudioJob J) {
    const int c = (int)(blockIdx.x / (unsigned)J.chain_len), j = (int)(blockIdx.x % (unsigned)J.chain_len);
    const int64_t s = c / J.cdiv, a = c % J.cdiv, out_row = s * J.out_a + j * J.out_c + a;
    int64_t row0;
    AudioCall k{-1, 0, 0};
    if (audio_chain(J, c, row0)) k = audio_call(J, c, row0, j);
    if (threadIdx.x == 0) J.n_out[out_row] = k.n_out;
    if (!k.n_out) return;
    const uint32_t *x = audio_pcm(J, row0, j);
    float2 *o = (float2 *)J.samples + out_row * J.out_pairs;
    if (k.f < 0) {
        for (int p = threadIdx.x; p < k.n_out; p += blockDim.x) o[p] = audio_scale(x[p]);
        return;
    }
    uint32_t h1, h2;
    audio_history(J, c, row0, j, k.f, k.f == 1 ? 2 : 1, h1, h2);
    const float *coef = J.coef + 5 * k.f;
    if (k.f == 1) audio_filter<2, 1>(x, o, k.n_out, h1, h2, coef);
    else if (k.f == 0) audio_filter<3, 1>(x, o, k.n_out, h1, h2, coef);
    else audio_filter<3, 2>(x, o, k.n_out, h1, h2, coef);
}

__global__ __launch_bounds__(64) void k_audio_state(AudioJob J) {
    const int t = blockIdx.x * 64 + threadIdx.x, c = t / 3, f = t - 3 * c;
    int64_t row0;
    if (c >= J.n_chains || !audio_chain(J, c, row0)) return;
    uint32_t h1, h2;
    audio_history(J, c, row0, J.chain_len, f, 2, h1, h2);
    uint32_t *S = J.state[c].hist[f];
    S[0] = h1;
    S[1] = h2;
}

hipError_t launch_audio(hipStream_t st, const AudioJob &J) {
    if (J.n_chains <= 0 || J.chain_len <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_audio_out, dim3((unsigned)J.n_chains * (unsigned)J.chain_len), dim3(256), 0, st, J);
    hipLaunchKernelGGL(k_audio_state, dim3((3u * (unsigned)J.n_chains + 63u) / 64u), dim3(64), 0, st, J);
    return hipGetLastError();
}

}  // namespace dab
