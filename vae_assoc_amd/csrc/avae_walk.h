// THE WALK of avae_ik.h as device code, shared by the kernels that walk the chain in registers (avae_ik.hip, avae_track.hip): every
// operation is the one avae_ik.h writes, in its order (tests/ik_reference.py restates them one by one).
#pragma once
#include "avae_device.h"

namespace avae {

#pragma clang fp contract(off)

// THE WALK's state: the tip (p, R) and, per joint, its origin o (turned into the Jacobian's J_v by jacobian_columns) and axis z.
// Every index is a compile-time constant once the loops are unrolled, so the arrays are registers.
template <int DC>
struct Walk {
    float p[3], R[9], o[DC][3], z[DC][3];
};

__device__ __forceinline__ void apply_frame(const float* f, float (&p)[3], float (&R)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = ((R[3 * r] * f[3] + R[3 * r + 1] * f[7]) + R[3 * r + 2] * f[11]) + p[r];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float r0 = R[3 * r], r1 = R[3 * r + 1], r2 = R[3 * r + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (r0 * f[c] + r1 * f[4 + c]) + r2 * f[8 + c];
    }
}

// ROUNDED: sin and cos are the double-precision functions of the float angle, rounded once -- the correctly rounded floats (but for
// double's own last bit), so the bits do not depend on which value within its ulp a float math library returns (avae_track.h)
template <int DC, bool ROUNDED = false>
__device__ __forceinline__ void walk(const float* frames_s, const float* axes_s, int D, const float (&q)[DC], Walk<DC>& w) {
#pragma unroll
    for (int i = 0; i < 9; ++i) w.R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
    w.p[0] = w.p[1] = w.p[2] = 0.0f;
#pragma unroll
    for (int j = 0; j < DC; ++j) {
        if (j < D) {
            // the constants are read from LDS where they are used: hoisted out of the solver's loops they would hold
            // 15 registers a joint for the whole kernel
            asm volatile("" ::: "memory");
            apply_frame(frames_s + 12 * j, w.p, w.R);
            const float ax = axes_s[3 * j], ay = axes_s[3 * j + 1], az = axes_s[3 * j + 2];
            float s, c;
            if (ROUNDED) {
                double sd, cd;
                sincos((double)q[j], &sd, &cd);
                s = (float)sd;
                c = (float)cd;
            } else {
                sincosf(q[j], &s, &c);
            }
            const float omc = 1.0f - c;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float r0 = w.R[3 * r], r1 = w.R[3 * r + 1], r2 = w.R[3 * r + 2];
                const float dot = (r0 * ax + r1 * ay) + r2 * az;
                w.o[j][r] = w.p[r];
                w.z[j][r] = dot;
                const float x0 = r1 * az - r2 * ay, x1 = r2 * ax - r0 * az, x2 = r0 * ay - r1 * ax;
                const float k = dot * omc;
                w.R[3 * r] = (r0 * c + x0 * s) + ax * k;
                w.R[3 * r + 1] = (r1 * c + x1 * s) + ay * k;
                w.R[3 * r + 2] = (r2 * c + x2 * s) + az * k;
            }
        }
    }
    apply_frame(frames_s + 12 * D, w.p, w.R);
}

// o_j <- J_v[:, j] = z_j x (p - o_j)
template <int DC>
__device__ __forceinline__ void jacobian_columns(int D, Walk<DC>& w) {
#pragma unroll
    for (int j = 0; j < DC; ++j) {
        if (j < D) {
            const float d0 = w.p[0] - w.o[j][0], d1 = w.p[1] - w.o[j][1], d2 = w.p[2] - w.o[j][2];
            const float z0 = w.z[j][0], z1 = w.z[j][1], z2 = w.z[j][2];
            w.o[j][0] = z1 * d2 - z2 * d1;
            w.o[j][1] = z2 * d0 - z0 * d2;
            w.o[j][2] = z0 * d1 - z1 * d0;
        }
    }
}

template <int DC>
__device__ __forceinline__ void load_chain(const float* frames, const float* axes, int D, float* frames_s, float* axes_s, int threads) {
    for (int i = threadIdx.x; i < (D + 1) * 12; i += threads) frames_s[i] = frames[i];
    for (int i = threadIdx.x; i < D * 3; i += threads) axes_s[i] = axes[i];
}

}  // namespace avae
