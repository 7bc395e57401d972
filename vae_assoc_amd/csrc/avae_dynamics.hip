// Joint-space inertia and inverse dynamics kernel (avae_dynamics.h, include/avae.h): k_motion_dynamics.
#include "avae_device.h"
#include "avae_dynamics.h"
#include "avae_walk.h"

namespace avae {

namespace {

// Every operation below is the one avae_dynamics.h writes, in its order: tests/dynamics_reference.py restates them one by one.
#pragma clang fp contract(off)

__device__ __forceinline__ void cross(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// world_s[quantity][joint][lane], col = world_s + lane: the quantities of joint j are kDynThreads * DC floats apart
enum { kO = 0, kZ = 3, kR = 6, kI = 9 };          // o_j, z_j, r_j (3 each), I_j (6: xx, xy, xz, yy, yz, zz)

template <int DC>
__device__ __forceinline__ void load3(const float* col, int quantity, int j, float (&x)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = col[((quantity + i) * DC + j) * kDynThreads];
}

// THE WALK WITH BODIES at the angles q[0 .. D) (LDS, the lane's row of the tile): o_j, z_j, r_j and I_j into the lane's columns.
// One trip per joint, not unrolled: nothing is indexed by j but LDS.  -> whether an angle is not finite
template <int DC>
__device__ __forceinline__ bool walk_bodies(const float* frames_s, const float* axes_s, const float* bodies_s, int D,
                                            const float* q, float* col) {
    float p[3] = {0.0f, 0.0f, 0.0f}, R[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
    bool bad = false;
#pragma unroll 1
    for (int j = 0; j < D; ++j) {
        apply_frame(frames_s + 12 * j, p, R);
        const float ax = axes_s[3 * j], ay = axes_s[3 * j + 1], az = axes_s[3 * j + 2];
        const float qj = q[j];
        bad = bad || !isfinite(qj);
        double sd, cd;
        sincos((double)qj, &sd, &cd);
        const float s = (float)sd, c = (float)cd;
        const float omc = 1.0f - c;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float r0 = R[3 * r], r1 = R[3 * r + 1], r2 = R[3 * r + 2];
            const float dot = (r0 * ax + r1 * ay) + r2 * az;
            col[((kO + r) * DC + j) * kDynThreads] = p[r];
            col[((kZ + r) * DC + j) * kDynThreads] = dot;
            const float x0 = r1 * az - r2 * ay, x1 = r2 * ax - r0 * az, x2 = r0 * ay - r1 * ax;
            const float k = dot * omc;
            R[3 * r] = (r0 * c + x0 * s) + ax * k;
            R[3 * r + 1] = (r1 * c + x1 * s) + ay * k;
            R[3 * r + 2] = (r2 * c + x2 * s) + az * k;
        }
        const float* b = bodies_s + kDynBody * j;
        const float L[3][3] = {{b[4], b[5], b[6]}, {b[5], b[7], b[8]}, {b[6], b[8], b[9]}};
        float A[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            col[((kR + i) * DC + j) * kDynThreads] = (R[3 * i] * b[1] + R[3 * i + 1] * b[2]) + R[3 * i + 2] * b[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) A[i][k] = (R[3 * i] * L[0][k] + R[3 * i + 1] * L[1][k]) + R[3 * i + 2] * L[2][k];
        }
        int slot = kI;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = i; k < 3; ++k)
                col[(slot++ * DC + j) * kDynThreads] = (A[i][0] * R[3 * k] + A[i][1] * R[3 * k + 1]) + A[i][2] * R[3 * k + 2];
        }
    }
    return bad;
}

// y = I_j x
template <int DC>
__device__ __forceinline__ void inertia_times(const float* col, int j, const float (&x)[3], float (&y)[3]) {
    float d[3], e[3];                                      // (xx, xy, xz), (yy, yz, zz)
    load3<DC>(col, kI, j, d);
    load3<DC>(col, kI + 3, j, e);
    y[0] = (d[0] * x[0] + d[1] * x[1]) + d[2] * x[2];
    y[1] = (d[1] * x[0] + e[0] * x[1]) + e[1] * x[2];
    y[2] = (d[2] * x[0] + e[1] * x[1]) + e[2] * x[2];
}

// THE PASS with a_j = u[j] (use_u) or the unit vector e's: tau_j, or NaN for a bad point, goes to out[j].  The joints' loops are
// unrolled so that F and N are registers; what a joint needs of the world comes from the lane's columns where it is used (a
// compiler barrier per joint keeps the loads from being hoisted out of the loop over the passes).
template <int DC>
__device__ __forceinline__ void newton_euler(const float* bodies_s, const float* col, int D, bool has_v, const float (&v)[DC],
                                             bool use_u, const float (&u)[DC], int e, const float (&g)[3], bool bad, float* out) {
    float F[DC][3], N[DC][3];
    float w[3] = {0.0f, 0.0f, 0.0f}, dw[3] = {0.0f, 0.0f, 0.0f}, ao[3] = {g[0], g[1], g[2]};
    float o[3], lo[3] = {0.0f, 0.0f, 0.0f}, z[3], r[3], d[3], t1[3], t2[3], t3[3];
#pragma unroll
    for (int j = 0; j < DC; ++j) {
        if (j < D) {
            asm volatile("" ::: "memory");
            const float aj = use_u ? u[j] : (j == e ? 1.0f : 0.0f);
            load3<DC>(col, kO, j, o);
            if (j > 0) {
#pragma unroll
                for (int i = 0; i < 3; ++i) d[i] = o[i] - lo[i];
                cross(dw, d, t1);
#pragma unroll
                for (int i = 0; i < 3; ++i) ao[i] = ao[i] + t1[i];
                if (has_v) {
                    cross(w, d, t2);
                    cross(w, t2, t3);
#pragma unroll
                    for (int i = 0; i < 3; ++i) ao[i] = ao[i] + t3[i];
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) lo[i] = o[i];
            load3<DC>(col, kZ, j, z);
#pragma unroll
            for (int i = 0; i < 3; ++i) t1[i] = dw[i] + z[i] * aj;
            if (has_v) {
                cross(w, z, t2);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    t1[i] = t1[i] + t2[i] * v[j];
                    w[i] = w[i] + z[i] * v[j];
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) dw[i] = t1[i];
            load3<DC>(col, kR, j, r);
            float ac[3];
            cross(dw, r, t1);
#pragma unroll
            for (int i = 0; i < 3; ++i) ac[i] = ao[i] + t1[i];
            if (has_v) {
                cross(w, r, t2);
                cross(w, t2, t3);
#pragma unroll
                for (int i = 0; i < 3; ++i) ac[i] = ac[i] + t3[i];
            }
            const float m = bodies_s[kDynBody * j];
#pragma unroll
            for (int i = 0; i < 3; ++i) F[j][i] = m * ac[i];
            inertia_times<DC>(col, j, dw, t1);
            if (has_v) {
                inertia_times<DC>(col, j, w, t2);
                cross(w, t2, t3);
#pragma unroll
                for (int i = 0; i < 3; ++i) t1[i] = t1[i] + t3[i];
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) N[j][i] = t1[i];
        }
    }
    float n[3] = {0.0f, 0.0f, 0.0f}, f[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = DC - 1; j >= 0; --j) {
        if (j < D) {
            asm volatile("" ::: "memory");
            load3<DC>(col, kO, j, o);
            load3<DC>(col, kR, j, r);
            load3<DC>(col, kZ, j, z);
            cross(r, F[j], t1);
            if (j == D - 1) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    n[i] = N[j][i] + t1[i];
                    f[i] = F[j][i];
                }
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i) d[i] = lo[i] - o[i];         // lo: o_(j+1)
                cross(d, f, t2);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    n[i] = ((N[j][i] + t1[i]) + n[i]) + t2[i];
                    f[i] = f[i] + F[j][i];
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) lo[i] = o[i];
            const float tau = (z[0] * n[0] + z[1] * n[1]) + z[2] * n[2];
            out[j] = bad ? __builtin_nanf("") : tau;
        }
    }
}

template <int DC>
__global__ __launch_bounds__(kDynThreads) void k_motion_dynamics(const DynArgs a) {
    constexpr int dp = DC | 1;
    __shared__ float io_s[kDynThreads * dp];
    __shared__ float world_s[kDynWorld * DC * kDynThreads];
    __shared__ float frames_s[(DC + 1) * 12];
    __shared__ float axes_s[DC * 3];
    __shared__ float bodies_s[DC * kDynBody];
    const int D = a.D, tid = threadIdx.x;
    load_chain<DC>(a.frames, a.axes, D, frames_s, axes_s, kDynThreads);
    for (int i = tid; i < D * kDynBody; i += kDynThreads) bodies_s[i] = a.bodies[i];
    float* col = world_s + tid;
    float* row = io_s + tid * dp;
    const long long tiles = (a.points + kDynThreads - 1) / kDynThreads;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long p0 = tile * kDynThreads;
        const int n = (int)(a.points - p0 < kDynThreads ? a.points - p0 : kDynThreads);
        // the tile's angles, speeds and accelerations come through io_s one after the other; the rows of a last tile's lanes
        // without a point hold zeros
        auto fetch = [&](const float* all) {
            __syncthreads();                               // io_s is read out; the first time: the constants are in
            const float* src = all + (size_t)p0 * D;
            for (int i = tid; i < kDynThreads * D; i += kDynThreads) {
                const int pt = i / D;
                io_s[pt * dp + (i - pt * D)] = i < n * D ? src[i] : 0.0f;
            }
            __syncthreads();
        };
        fetch(a.traj);
        bool bad = walk_bodies<DC>(frames_s, axes_s, bodies_s, D, row, col);
        float v[DC], u[DC];
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            const float* all = which == 0 ? a.vel : a.acc;
            float(&x)[DC] = which == 0 ? v : u;
            if (all) fetch(all);
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                x[c] = (all && c < D) ? row[c] : 0.0f;
                bad = bad || !isfinite(x[c]);
            }
        }
        // pass 0 gravity, 1 coriolis, 2 torque, 3 + j column j of the inertia
        const int passes = a.inertia ? 3 + D : 3;
#pragma unroll 1
        for (int p = 0; p < passes; ++p) {
            float* out = p == 0 ? a.gravity : p == 1 ? a.coriolis : p == 2 ? a.torque : a.inertia;
            if (!out) continue;
            const bool has_v = (p == 1 || p == 2) && a.vel != nullptr;
            const bool falls = p == 0 || p == 2;
            const float start[3] = {falls ? a.g[0] : 0.0f, falls ? a.g[1] : 0.0f, falls ? a.g[2] : 0.0f};
            __syncthreads();                               // io_s is read out
            newton_euler<DC>(bodies_s, col, D, has_v, v, p == 2, u, p - 3, start, bad, row);
            __syncthreads();
            if (p < 3) {
                float* dst = out + (size_t)p0 * D;
                for (int i = tid; i < n * D; i += kDynThreads) {
                    const int pt = i / D;
                    dst[i] = io_s[pt * dp + (i - pt * D)];
                }
            } else {
                const int j = p - 3, len = j + 1;
                for (int i = tid; i < n * len; i += kDynThreads) {
                    const int pt = i / len, c = i - pt * len;
                    float* M = out + (size_t)(p0 + pt) * D * D;
                    const float x = io_s[pt * dp + c];
                    M[j * D + c] = x;
                    M[c * D + j] = x;
                }
            }
        }
    }
}

}  // namespace

void launch_motion_dynamics(const DynArgs& a, hipStream_t s) {
    const long long tiles = (a.points + kDynThreads - 1) / kDynThreads;
    const dim3 grid((unsigned)std::min<long long>(tiles, 1 << 20)), block(kDynThreads);
    if (a.D <= 4) launch_kernel(k_motion_dynamics<4>, grid, block, 0, s, a);
    else if (a.D <= 8) launch_kernel(k_motion_dynamics<8>, grid, block, 0, s, a);
    else launch_kernel(k_motion_dynamics<16>, grid, block, 0, s, a);
}

}  // namespace avae
