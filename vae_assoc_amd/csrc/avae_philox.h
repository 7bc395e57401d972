// The library's random stream: Philox4x32-10 blocks and the Box-Muller normals formed from them.  One definition for every kernel
// that draws (the eps and corruption streams of avae_kernels.hip, the search stream of avae_search.hip): what differs between
// the streams is the counter and the key alone, documented at each stream in include/avae.h.
#pragma once
#include <hip/hip_runtime.h>

namespace avae {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                              unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
        const unsigned n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        const unsigned n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// four N(0,1) from one Philox block
__device__ __forceinline__ void box_muller4(const unsigned r[4], float n[4]) {
    // Box-Muller on (0,1) uniforms built from the top 24 bits; the logarithm is the hardware's (v_log_f32, ~1 ulp)
    const float u0 = ((r[0] >> 8) + 0.5f) * (1.0f / 16777216.0f), u1 = ((r[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((r[2] >> 8) + 0.5f) * (1.0f / 16777216.0f), u3 = ((r[3] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float ra = sqrtf(-2.0f * __logf(u0)), rb = sqrtf(-2.0f * __logf(u2));
    // v_sin_f32 / v_cos_f32 take their argument in revolutions: sin(2*pi*u) directly
    n[0] = ra * __builtin_amdgcn_cosf(u1); n[1] = ra * __builtin_amdgcn_sinf(u1);
    n[2] = rb * __builtin_amdgcn_cosf(u3); n[3] = rb * __builtin_amdgcn_sinf(u3);
}

}  // namespace avae
