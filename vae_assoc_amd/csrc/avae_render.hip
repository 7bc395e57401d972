// Pen-path kinematics and stroke rendering kernels (avae_render.h, include/avae.h): k_motion_fk, k_stroke_render.
#include "avae_render_dev.h"

namespace avae {

namespace {

// Every operation below is the one written (a fused multiply-add only where __builtin_fmaf says so): tests/render_reference.py
// restates them one by one.
#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------ forward kinematics
__global__ __launch_bounds__(kRenderThreads) void k_motion_fk(const FkArgs a) {
    __shared__ float q_s[kRenderThreads * (kFkMaxD | 1)];
    __shared__ float p_s[kRenderThreads * 3];
    __shared__ float frames_s[(kFkMaxD + 1) * 12];
    __shared__ float axes_s[kFkMaxD * 3];
    const int D = a.D, dp = D | 1, tid = threadIdx.x;
    for (int i = tid; i < (D + 1) * 12; i += kRenderThreads) frames_s[i] = a.frames[i];
    for (int i = tid; i < D * 3; i += kRenderThreads) axes_s[i] = a.axes[i];
    const long long tiles = (a.points + kRenderThreads - 1) / kRenderThreads;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long p0 = tile * kRenderThreads;
        const int n = (int)(a.points - p0 < kRenderThreads ? a.points - p0 : kRenderThreads);
        __syncthreads();                                   // the previous tile is written out; the first time: nothing to wait for
        const float* src = a.traj + (size_t)p0 * D;
        for (int i = tid; i < n * D; i += kRenderThreads) {
            const int pt = i / D;
            q_s[pt * dp + (i - pt * D)] = src[i];
        }
        __syncthreads();
        if (tid < n) {
            const float* q = q_s + tid * dp;
            float vx = frames_s[D * 12 + 3], vy = frames_s[D * 12 + 7], vz = frames_s[D * 12 + 11];
            for (int j = D - 1; j >= 0; --j) {
                float s, c;
                sincosf(q[j], &s, &c);
                const float ax = axes_s[3 * j], ay = axes_s[3 * j + 1], az = axes_s[3 * j + 2];
                const float cx = ay * vz - az * vy, cy = az * vx - ax * vz, cz = ax * vy - ay * vx;
                const float k = ((ax * vx + ay * vy) + az * vz) * (1.0f - c);
                const float wx = (vx * c + cx * s) + ax * k, wy = (vy * c + cy * s) + ay * k, wz = (vz * c + cz * s) + az * k;
                const float* f = frames_s + j * 12;
                vx = ((f[0] * wx + f[1] * wy) + f[2] * wz) + f[3];
                vy = ((f[4] * wx + f[5] * wy) + f[6] * wz) + f[7];
                vz = ((f[8] * wx + f[9] * wy) + f[10] * wz) + f[11];
            }
            p_s[3 * tid] = vx; p_s[3 * tid + 1] = vy; p_s[3 * tid + 2] = vz;
        }
        __syncthreads();
        float* dst = a.path + (size_t)p0 * 3;
        for (int i = tid; i < n * 3; i += kRenderThreads) dst[i] = p_s[i];
    }
}

// ------------------------------------------------------------------------------------------------ stroke rendering
// (the row's forward pass is render_row of avae_render_dev.h, which the reverse pass of avae_grad.hip calls too)
template <int SS>
__global__ __launch_bounds__(kRenderThreads) void k_stroke_render(const RenderArgs a) {
    extern __shared__ __align__(16) float render_smem[];
    render_row<SS>(a, render_smem, render_lds(a.T, a.H), a.image != nullptr || a.img_l2 != nullptr, a.img_l2 != nullptr,
                   a.height_l2 != nullptr);
}

}  // namespace

void launch_motion_fk(const FkArgs& a, hipStream_t s) {
    const long long tiles = (a.points + kRenderThreads - 1) / kRenderThreads;
    launch_kernel(k_motion_fk, dim3((unsigned)std::min<long long>(tiles, 1 << 20)), dim3(kRenderThreads), 0, s, a);
}

void launch_stroke_render(const RenderArgs& a, long long rows, hipStream_t s) {
    const dim3 grid((unsigned)rows), block(kRenderThreads);
    const size_t lds = render_lds_bytes(a.T, a.H);
    switch (a.ss) {
        case 1: launch_kernel(k_stroke_render<1>, grid, block, lds, s, a); break;
        case 2: launch_kernel(k_stroke_render<2>, grid, block, lds, s, a); break;
        case 4: launch_kernel(k_stroke_render<4>, grid, block, lds, s, a); break;
        default: launch_kernel(k_stroke_render<8>, grid, block, lds, s, a); break;
    }
}

}  // namespace avae
