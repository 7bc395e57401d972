// Pose, Jacobian and inverse kinematics kernels (avae_ik.h, include/avae.h): k_motion_pose, k_motion_ik.
#include "avae_device.h"
#include "avae_ik.h"
#include "avae_walk.h"

namespace avae {

namespace {

// Every operation below is the one avae_ik.h writes, in its order: tests/ik_reference.py restates them one by one.
#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------ pose and Jacobian
template <int DC>
__global__ __launch_bounds__(kPoseThreads) void k_motion_pose(const PoseArgs a) {
    constexpr int dp = DC | 1;
    __shared__ float q_s[kPoseThreads * dp];
    __shared__ float out_s[kPoseThreads * 12];
    __shared__ float frames_s[(DC + 1) * 12];
    __shared__ float axes_s[DC * 3];
    const int D = a.D, tid = threadIdx.x;
    load_chain<DC>(a.frames, a.axes, D, frames_s, axes_s, kPoseThreads);
    float* pos_s = out_s;
    float* rot_s = out_s + kPoseThreads * 3;
    const long long tiles = (a.points + kPoseThreads - 1) / kPoseThreads;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long p0 = tile * kPoseThreads;
        const int n = (int)(a.points - p0 < kPoseThreads ? a.points - p0 : kPoseThreads);
        __syncthreads();                                   // the previous tile is written out; the first time: the constants are in
        const float* src = a.traj + (size_t)p0 * D;
        for (int i = tid; i < n * D; i += kPoseThreads) {
            const int pt = i / D;
            q_s[pt * dp + (i - pt * D)] = src[i];
        }
        __syncthreads();
        if (tid < n) {
            float q[DC];
#pragma unroll
            for (int c = 0; c < DC; ++c) q[c] = c < D ? q_s[tid * dp + c] : 0.0f;
            Walk<DC> w;
            walk<DC>(frames_s, axes_s, D, q, w);
#pragma unroll
            for (int r = 0; r < 3; ++r) pos_s[3 * tid + r] = w.p[r];
#pragma unroll
            for (int i = 0; i < 9; ++i) rot_s[9 * tid + i] = w.R[i];
            if (a.jacobian) {
                jacobian_columns<DC>(D, w);
                float* J = a.jacobian + (size_t)(p0 + tid) * 6 * D;
#pragma unroll
                for (int c = 0; c < DC; ++c) {
                    if (c < D) {
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            J[r * D + c] = w.o[c][r];
                            J[(3 + r) * D + c] = w.z[c][r];
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (a.position) {
            float* dst = a.position + (size_t)p0 * 3;
            for (int i = tid; i < n * 3; i += kPoseThreads) dst[i] = pos_s[i];
        }
        if (a.rotation) {
            float* dst = a.rotation + (size_t)p0 * 9;
            for (int i = tid; i < n * 9; i += kPoseThreads) dst[i] = rot_s[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------ inverse kinematics
template <int DC, int M>
__global__ __launch_bounds__(kIkThreads) void k_motion_ik(const IkArgs a) {
    __shared__ float frames_s[(DC + 1) * 12];
    __shared__ float axes_s[DC * 3];
    __shared__ float lim_s[DC * 2];
    const int D = a.D, T = a.T, tid = threadIdx.x;
    const bool clamp = a.limits != nullptr;
    load_chain<DC>(a.frames, a.axes, D, frames_s, axes_s, kIkThreads);
    if (clamp)
        for (int i = tid; i < 2 * D; i += kIkThreads) lim_s[i] = a.limits[i];
    __syncthreads();
    const long long row = (long long)blockIdx.x * kIkThreads + tid;
    if (row >= a.rows) return;

    const float nan = __builtin_nanf("");
    float q[DC];
    bool bad_seed = false;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
        q[c] = c < D ? a.seed[(size_t)row * D + c] : 0.0f;
        bad_seed = bad_seed || !isfinite(q[c]);
    }
    float G[9];
    if (M == 6) {
        const float* g = a.orient + (a.orient_per_row ? (size_t)row * 9 : 0);
#pragma unroll
        for (int i = 0; i < 9; ++i) G[i] = g[i];
    }
    const float damp2 = a.damping * a.damping;

    for (int t = 0; t < T; ++t) {
        const size_t pt = (size_t)row * T + t;
        const float g0 = a.path[pt * 3], g1 = a.path[pt * 3 + 1], g2 = a.path[pt * 3 + 2];
        const bool bad = bad_seed || !(isfinite(g0) && isfinite(g1) && isfinite(g2));
        int status = 3, iters = 0;
        float res = nan, rres = nan;
        if (!bad) {
            for (int k = 0;; ++k) {
                Walk<DC> w;
                walk<DC>(frames_s, axes_s, D, q, w);
                float e[M];
                e[0] = g0 - w.p[0]; e[1] = g1 - w.p[1]; e[2] = g2 - w.p[2];
                res = sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
                bool done = res < a.tol;
                if (M == 6) {
                    // sum over the columns i of R x G, column i of R = (R[i], R[3 + i], R[6 + i])
                    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const float r0 = w.R[i], r1 = w.R[3 + i], r2 = w.R[6 + i], h0 = G[i], h1 = G[3 + i], h2 = G[6 + i];
                        const float x0 = r1 * h2 - r2 * h1, x1 = r2 * h0 - r0 * h2, x2 = r0 * h1 - r1 * h0;
                        s0 = i == 0 ? x0 : s0 + x0;
                        s1 = i == 0 ? x1 : s1 + x1;
                        s2 = i == 0 ? x2 : s2 + x2;
                    }
                    e[M - 3] = 0.5f * s0; e[M - 2] = 0.5f * s1; e[M - 1] = 0.5f * s2;
                    rres = sqrtf((e[M - 3] * e[M - 3] + e[M - 2] * e[M - 2]) + e[M - 1] * e[M - 1]);
                    done = done && rres < a.rot_tol;
                }
                iters = k;
                if (done) { status = 0; break; }
                if (k == a.n_iters) { status = 1; break; }
                jacobian_columns<DC>(D, w);
                // J[i][c]: i < 3 the row i of J_v, else of J_w
#define AVAE_IK_J(i, c) ((i) < 3 ? w.o[c][(i) < 3 ? (i) : 0] : w.z[c][(i) < 3 ? 0 : (i) - 3])
                float L[M][M];
#pragma unroll
                for (int c = 0; c < DC; ++c) {
                    if (c < D) {
#pragma unroll
                        for (int i = 0; i < M; ++i) {
#pragma unroll
                            for (int j = 0; j <= i; ++j) {
                                const float x = AVAE_IK_J(i, c) * AVAE_IK_J(j, c);
                                L[i][j] = c == 0 ? x : L[i][j] + x;
                            }
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < M; ++i) L[i][i] = L[i][i] + damp2;
                bool pivot = true;
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    float s = L[j][j];
#pragma unroll
                    for (int kk = 0; kk < j; ++kk) s = s - L[j][kk] * L[j][kk];
                    pivot = pivot && (s > 0.0f);
                    const float d = sqrtf(s);
                    L[j][j] = d;
#pragma unroll
                    for (int i = j + 1; i < M; ++i) {
                        float v = L[i][j];
#pragma unroll
                        for (int kk = 0; kk < j; ++kk) v = v - L[i][kk] * L[j][kk];
                        L[i][j] = v / d;
                    }
                }
                if (!pivot) { status = 2; break; }
                float y[M];
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    float v = e[i];
#pragma unroll
                    for (int kk = 0; kk < i; ++kk) v = v - L[i][kk] * y[kk];
                    y[i] = v / L[i][i];
                }
#pragma unroll
                for (int i = M - 1; i >= 0; --i) {
                    float v = y[i];
#pragma unroll
                    for (int kk = M - 1; kk > i; --kk) v = v - L[kk][i] * y[kk];
                    y[i] = v / L[i][i];
                }
                float dq[DC], big = 0.0f;
#pragma unroll
                for (int c = 0; c < DC; ++c) {
                    dq[c] = 0.0f;
                    if (c < D) {
                        float v = AVAE_IK_J(0, c) * y[0];
#pragma unroll
                        for (int i = 1; i < M; ++i) v = v + AVAE_IK_J(i, c) * y[i];
                        dq[c] = v;
                        big = fmaxf(big, fabsf(v));
                    }
                }
#undef AVAE_IK_J
                const bool shrink = big > a.max_step;
                const float f = a.max_step / big;
                // dq <- q + dq; the step is committed only when every new angle is finite (fmaxf above drops a NaN and the
                // clamp below would turn one into lo: neither may decide).  x * 0 is +-0 for a finite x and NaN otherwise, so
                // one running sum tests them all: a flag per angle costs <16, 3> its second wave per SIMD (256 + 20 AGPRs)
                float zero = 0.0f;
#pragma unroll
                for (int c = 0; c < DC; ++c) {
                    if (c < D) {
                        const float v = shrink ? dq[c] * f : dq[c];
                        dq[c] = q[c] + v;
                        zero = zero + dq[c] * 0.0f;
                    }
                }
                if (!(zero == 0.0f)) { status = 2; break; }
#pragma unroll
                for (int c = 0; c < DC; ++c) {
                    if (c < D) {
                        float x = dq[c];
                        if (clamp) x = fminf(fmaxf(x, lim_s[2 * c]), lim_s[2 * c + 1]);
                        q[c] = x;
                    }
                }
            }
        }
        float* out = a.traj + pt * D;
#pragma unroll
        for (int c = 0; c < DC; ++c)
            if (c < D) out[c] = bad ? nan : q[c];
        if (a.residual) a.residual[pt] = res;
        if (a.rot_residual) a.rot_residual[pt] = rres;
        if (a.iterations) a.iterations[pt] = iters;
        if (a.status) a.status[pt] = status;
    }
}

template <int DC>
void launch_ik_class(const IkArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.rows + kIkThreads - 1) / kIkThreads)), block(kIkThreads);
    if (a.orient) launch_kernel(k_motion_ik<DC, 6>, grid, block, 0, s, a);
    else launch_kernel(k_motion_ik<DC, 3>, grid, block, 0, s, a);
}

}  // namespace

void launch_motion_pose(const PoseArgs& a, hipStream_t s) {
    const long long tiles = (a.points + kPoseThreads - 1) / kPoseThreads;
    const dim3 grid((unsigned)std::min<long long>(tiles, 1 << 20)), block(kPoseThreads);
    if (a.D <= 4) launch_kernel(k_motion_pose<4>, grid, block, 0, s, a);
    else if (a.D <= 8) launch_kernel(k_motion_pose<8>, grid, block, 0, s, a);
    else launch_kernel(k_motion_pose<16>, grid, block, 0, s, a);
}

void launch_motion_ik(const IkArgs& a, hipStream_t s) {
    if (a.D <= 4) launch_ik_class<4>(a, s);
    else if (a.D <= 8) launch_ik_class<8>(a, s);
    else launch_ik_class<16>(a, s);
}

}  // namespace avae
