// Gradients through the writing chain (avae_grad.h, include/avae.h): k_stroke_render_vjp, k_motion_fk_vjp,
// k_motion_eval_vjp, k_rows_adam.
#include "avae_render_dev.h"
#include "avae_grad.h"

namespace avae {

namespace {

// Every operation below is the one written (a fused multiply-add only where __builtin_fmaf says so): tests/render_grad_reference.py
// restates them one by one.
#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------ the renderer's reverse pass
__device__ __forceinline__ long long to_fixed(float x, double scale) { return __double2ll_rn((double)x * scale); }
__device__ __forceinline__ void fixed_add(long long* at, long long x) {
    atomicAdd(reinterpret_cast<unsigned long long*>(at), (unsigned long long)x);          // integer: exact in any order
}

template <int SS>
__global__ __launch_bounds__(kRenderThreads) void k_stroke_render_vjp(const RenderVjpArgs a) {
    extern __shared__ __align__(16) float render_smem[];
    const RenderArgs& fa = a.f;
    const int T = fa.T, H = fa.H, npx = H * H, nseg = T > 1 ? T - 1 : 1, tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const RenderLds l = render_lds(T, H);
    const RenderVjpLds lv = render_vjp_lds(T, H);
    const bool img_part = a.g_image != nullptr || a.g_img_l2 != nullptr;
    const bool want_l2 = fa.img_l2 != nullptr || a.g_img_l2 != nullptr, want_h = fa.height_l2 != nullptr || a.g_height_l2 != nullptr;
    const RenderRow st = render_row<SS>(fa, render_smem, l, fa.image != nullptr || want_l2 || img_part, want_l2, want_h);
    float* gp = a.grad_path + row * (size_t)T * 3;
    const float nan = __builtin_nanf("");
    if (st.bad) {                                          // (uniform) the forward wrote its NaNs
        for (int i = tid; i < 3 * T; i += kRenderThreads) gp[i] = nan;
        if (a.objective && tid == 0) a.objective[row] = nan;
        return;
    }
    if (a.objective && tid == 0) {
        float o = a.g_img_l2 ? a.g_img_l2[row] * st.img_l2 : 0.0f;
        if (a.g_height_l2) o = __builtin_fmaf(a.g_height_l2[row], st.height_l2, o);
        a.objective[row] = o;
    }

    const float4* seg = reinterpret_cast<const float4*>(render_smem + l.seg);
    const float *inv = render_smem + l.inv, *cu = render_smem + l.cu, *cv = render_smem + l.cv;
    float *img = render_smem + l.img, *red = render_smem + l.red;
    const unsigned short* list = reinterpret_cast<const unsigned short*>(render_smem + l.list);
    long long* accu = reinterpret_cast<long long*>(render_smem + lv.accu);
    long long* accv = reinterpret_cast<long long*>(render_smem + lv.accv);
    long long* slots = reinterpret_cast<long long*>(render_smem + lv.slots);
    constexpr int kPts = kRenderMaxT / kRenderThreads;
    constexpr float kInvArea = 1.0f / (float)(SS * SS);
    const Frame f = st.f;
    const float hs = (float)(H * SS);

    bool poisoned = false, live = false;                   // (uniform) a non-finite cotangent / a cotangent that is not 0
    float bound = 0.0f;
    if (img_part && T > 1) {                               // (uniform) T = 1: the image part is 0 by definition
        // a. the pixels' cotangents
        const float gl2 = a.g_img_l2 ? a.g_img_l2[row] : 0.0f;
        const bool use_l2 = a.g_img_l2 != nullptr && st.img_l2 != 0.0f;
        float bsum[1] = {0.0f};
        for (int p = tid; p < npx; p += kRenderThreads) {
            float g = a.g_image ? a.g_image[row * npx + p] : 0.0f;
            if (use_l2) g = g + (gl2 * (img[p] - fa.target[row * npx + p])) / st.img_l2;
            g = g * kInvArea;
            img[p] = g;
            bsum[0] = bsum[0] + fabsf(g);
        }
        const int op[1] = {kSum};
        block_tree<1>(red, bsum, op);                      // (its barriers also publish the cotangents)
        bound = (bsum[0] * (float)(SS * SS)) / f.delta;
        poisoned = !latent_finite(bound);
        live = !poisoned && bound > 0.0f;
    }

    int ext[4] = {-1, -1, -1, -1};                         // first argmin u, argmax u, argmin v, argmax v
    double inv_scale = 0.0;
    float gctr_u = 0.0f, gctr_v = 0.0f, gW = 0.0f;
    if (live) {
        // b. the extreme points (a thread's points from the last to the first, so the first match stays)
        float idx[4] = {__builtin_inff(), __builtin_inff(), __builtin_inff(), __builtin_inff()};
#pragma unroll
        for (int j = kPts - 1; j >= 0; --j) {
            const int t = tid + j * kRenderThreads;
            if (t < T) {
                if (cu[t] == st.box[0]) idx[0] = (float)t;
                if (cu[t] == st.box[1]) idx[1] = (float)t;
                if (cv[t] == st.box[2]) idx[2] = (float)t;
                if (cv[t] == st.box[3]) idx[3] = (float)t;
            }
        }
        const int op[4] = {kMin, kMin, kMin, kMin};
        block_tree<4>(red, idx, op);
#pragma unroll
        for (int k = 0; k < 4; ++k) ext[k] = (int)idx[k];

        // c. the samples
        int e2;
        (void)frexpf(bound, &e2);                          // bound = m * 2^e2, m in [0.5, 1)
        const double scale = ldexp(1.0, 60 - e2);
        inv_scale = ldexp(1.0, e2 - 60);
        for (int t = tid; t < T; t += kRenderThreads) { accu[t] = 0; accv[t] = 0; }
        if (tid < 4) slots[tid] = 0;
        __syncthreads();
        long long s_cu = 0, s_cv = 0, s_w = 0, s_d = 0;
        for (int it = tid; it < st.items; it += kRenderThreads) {
            const int pix = list[it / SS], sa = it % SS, i = pix / H, j = pix - i * H;
            const float arow = (float)(i * SS + sa) + 0.5f;
            const float v = __builtin_fmaf(-arow, f.delta, f.v0);
            float u[SS], m[SS];
            int js[SS];
#pragma unroll
            for (int b = 0; b < SS; ++b) {
                u[b] = __builtin_fmaf((float)(j * SS + b) + 0.5f, f.delta, f.u0);
                m[b] = __builtin_inff();
                js[b] = 0;
            }
            for (int s = 0; s < nseg; ++s) {
                const float4 g = seg[s];
                const float iv = inv[s], py = v - g.y, pydy = py * g.w;
#pragma unroll
                for (int b = 0; b < SS; ++b) {
                    const float d2 = seg_dist2(u[b], py, pydy, g, iv);
                    if (d2 < m[b]) { m[b] = d2; js[b] = s; }
                }
            }
            const float gcov = img[pix], alpha_a = arow / hs - 0.5f;
#pragma unroll
            for (int b = 0; b < SS; ++b) {
                const float d = sqrtf(m[b]), q = (f.r - d) / f.delta, x = 0.5f + q;
                if (!(x > 0.0f && x < 1.0f)) continue;
                const int s = js[b];
                const float4 g = seg[s];
                const float px = u[b] - g.x, py = v - g.y;
                float t = __builtin_fmaf(px, g.z, py * g.w) * inv[s];
                t = fminf(fmaxf(t, 0.0f), 1.0f);
                const float ex = __builtin_fmaf(-t, g.z, px), ey = __builtin_fmaf(-t, g.w, py);
                const float gd = -gcov / f.delta;
                const float nx = d > 0.0f ? ex / d : 0.0f, ny = d > 0.0f ? ey / d : 0.0f;
                const float gsx = gd * nx, gsy = gd * ny, wa = 1.0f - t;
                const float alpha_b = ((float)(j * SS + b) + 0.5f) / hs - 0.5f;
                fixed_add(accu + s, to_fixed(-(wa * gsx), scale));
                fixed_add(accv + s, to_fixed(-(wa * gsy), scale));
                fixed_add(accu + s + 1, to_fixed(-(t * gsx), scale));
                fixed_add(accv + s + 1, to_fixed(-(t * gsy), scale));
                s_cu += to_fixed(gsx, scale);
                s_cv += to_fixed(gsy, scale);
                s_w += to_fixed(gsx * alpha_b - gsy * alpha_a, scale);
                s_d += to_fixed(-((q / f.delta) * gcov), scale);
            }
        }
        fixed_add(slots, s_cu); fixed_add(slots + 1, s_cv); fixed_add(slots + 2, s_w); fixed_add(slots + 3, s_d);
        __syncthreads();
        gctr_u = (float)((double)slots[0] * inv_scale);
        gctr_v = (float)((double)slots[1] * inv_scale);
        gW = (float)((double)slots[2] * inv_scale) + (float)((double)slots[3] * inv_scale) / hs;
    }

    // d. the points
    const float* pl = fa.plane;
    const float* path = fa.path + row * (size_t)T * 3;
    const float hgt = want_h ? fa.height[row] : 0.0f;
    const bool h_part = a.g_height_l2 != nullptr && st.height_l2 != 0.0f;
    const float gh = h_part ? a.g_height_l2[row] : 0.0f;
    const float kW = (1.0f + fa.margin) * gW, hu = 0.5f * gctr_u, hv = 0.5f * gctr_v;
    for (int t = tid; t < T; t += kRenderThreads) {
        float gcu = 0.0f, gcv = 0.0f;
        if (live) {
            gcu = (float)((double)accu[t] * inv_scale);
            gcv = (float)((double)accv[t] * inv_scale);
            if (t == ext[1]) gcu = gcu + hu;
            if (t == ext[0]) gcu = gcu + hu;
            if (t == ext[3]) gcv = gcv + hv;
            if (t == ext[2]) gcv = gcv + hv;
            if (st.longer_u) {
                if (t == ext[1]) gcu = gcu + kW;
                if (t == ext[0]) gcu = gcu - kW;
            } else {
                if (t == ext[3]) gcv = gcv + kW;
                if (t == ext[2]) gcv = gcv - kW;
            }
        }
        if (poisoned) { gcu = nan; gcv = nan; }
        float gx = __builtin_fmaf(gcv, pl[3], gcu * pl[0]);
        float gy = __builtin_fmaf(gcv, pl[4], gcu * pl[1]);
        float gz = __builtin_fmaf(gcv, pl[5], gcu * pl[2]);
        if (h_part) {
            const float e = __builtin_fmaf(pl[8], path[3 * t + 2], __builtin_fmaf(pl[7], path[3 * t + 1], pl[6] * path[3 * t])) - hgt;
            const float k = (gh * e) / st.height_l2;
            gx = __builtin_fmaf(k, pl[6], gx); gy = __builtin_fmaf(k, pl[7], gy); gz = __builtin_fmaf(k, pl[8], gz);
        }
        gp[3 * t] = gx; gp[3 * t + 1] = gy; gp[3 * t + 2] = gz;
    }
}

// ------------------------------------------------------------------------------------------------ forward kinematics, reversed
// x -> Rot(a, -q) x = (x c - (a x x) s) + a ((a . x)(1 - c))
__device__ __forceinline__ void rot_back(float ax, float ay, float az, float s, float c, float& x, float& y, float& z) {
    const float cx = ay * z - az * y, cy = az * x - ax * z, cz = ax * y - ay * x;
    const float k = ((ax * x + ay * y) + az * z) * (1.0f - c);
    const float rx = (x * c - cx * s) + ax * k, ry = (y * c - cy * s) + ay * k, rz = (z * c - cz * s) + az * k;
    x = rx; y = ry; z = rz;
}

__global__ __launch_bounds__(kRenderThreads) void k_motion_fk_vjp(const FkVjpArgs a) {
    __shared__ float q_s[kRenderThreads * (kFkMaxD | 1)];          // the angles, then their gradients
    __shared__ float sn_s[kRenderThreads * (kFkMaxD | 1)];
    __shared__ float cs_s[kRenderThreads * (kFkMaxD | 1)];
    __shared__ float g_s[kRenderThreads * 3];
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
        const float* gsrc = a.grad_path + (size_t)p0 * 3;
        for (int i = tid; i < n * 3; i += kRenderThreads) g_s[i] = gsrc[i];
        __syncthreads();
        if (tid < n) {
            float* q = q_s + tid * dp;
            float *sn = sn_s + tid * dp, *cs = cs_s + tid * dp;
            // inwards, as k_motion_fk
            float vx = frames_s[D * 12 + 3], vy = frames_s[D * 12 + 7], vz = frames_s[D * 12 + 11];
            for (int j = D - 1; j >= 0; --j) {
                float s, c;
                sincosf(q[j], &s, &c);
                sn[j] = s; cs[j] = c;
                const float ax = axes_s[3 * j], ay = axes_s[3 * j + 1], az = axes_s[3 * j + 2];
                const float cx = ay * vz - az * vy, cy = az * vx - ax * vz, cz = ax * vy - ay * vx;
                const float k = ((ax * vx + ay * vy) + az * vz) * (1.0f - c);
                const float wx = (vx * c + cx * s) + ax * k, wy = (vy * c + cy * s) + ay * k, wz = (vz * c + cz * s) + az * k;
                const float* f = frames_s + j * 12;
                vx = ((f[0] * wx + f[1] * wy) + f[2] * wz) + f[3];
                vy = ((f[4] * wx + f[5] * wy) + f[6] * wz) + f[7];
                vz = ((f[8] * wx + f[9] * wy) + f[10] * wz) + f[11];
            }
            // outwards, the tip and the cotangent in joint j's frame
            float hx = g_s[3 * tid], hy = g_s[3 * tid + 1], hz = g_s[3 * tid + 2];
            for (int j = 0; j < D; ++j) {
                const float* f = frames_s + j * 12;
                const float dx = vx - f[3], dy = vy - f[7], dz = vz - f[11];
                float wx = (f[0] * dx + f[4] * dy) + f[8] * dz, wy = (f[1] * dx + f[5] * dy) + f[9] * dz;
                float wz = (f[2] * dx + f[6] * dy) + f[10] * dz;
                float kx = (f[0] * hx + f[4] * hy) + f[8] * hz, ky = (f[1] * hx + f[5] * hy) + f[9] * hz;
                float kz = (f[2] * hx + f[6] * hy) + f[10] * hz;
                const float ax = axes_s[3 * j], ay = axes_s[3 * j + 1], az = axes_s[3 * j + 2];
                const float cx = ay * wz - az * wy, cy = az * wx - ax * wz, cz = ax * wy - ay * wx;
                q[j] = (cx * kx + cy * ky) + cz * kz;
                const float s = sn[j], c = cs[j];
                rot_back(ax, ay, az, s, c, wx, wy, wz);
                rot_back(ax, ay, az, s, c, kx, ky, kz);
                vx = wx; vy = wy; vz = wz; hx = kx; hy = ky; hz = kz;
            }
        }
        __syncthreads();
        float* dst = a.grad_traj + (size_t)p0 * D;
        for (int i = tid; i < n * D; i += kRenderThreads) {
            const int pt = i / D;
            dst[i] = q_s[pt * dp + (i - pt * D)];
        }
    }
}

// ------------------------------------------------------------------------------------------------ motion decoding, reversed
__global__ __launch_bounds__(kMotionThreads) void k_motion_eval_vjp(const MotionVjpArgs a) {
    constexpr int kLd = kFitSlab + 1, kKp = kMotionMaxKb | 1;
    __shared__ float phi_s[kMotionMaxKb * kLd];                            // [k][t]
    __shared__ float th_s[kMotionRows * kMotionMaxD * kKp];                // [b][d][k], rows of odd length
    __shared__ float g_s[kMotionRows * kFitSlab * kMotionMaxD];            // the gradients that pass, [b][t][d]
    __shared__ float gain_s[kFitSlab * kMotionMaxNc];
    __shared__ float tgt_s[kMotionRows * kMotionMaxD * kMotionMaxNc];
    const int D = a.D, Kb = a.Kb, T = a.T, nc = a.nc, P = D * Kb, kp = Kb | 1, tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * kMotionRows;
    const int nb = (int)(a.rows - r0 < kMotionRows ? a.rows - r0 : kMotionRows);
    const bool limited = a.limits != nullptr;
    if (limited) {
        for (int e = tid; e < nb * P; e += kMotionThreads) {
            const int b = e / P, j = e - b * P, d = j / Kb, k = j - d * Kb;
            th_s[(b * D + d) * kp + k] = __builtin_fmaf(a.params[(size_t)r0 * P + e], a.scale ? a.scale[j] : 1.0f, a.shift ? a.shift[j] : 0.0f);
        }
        for (int i = tid; i < nb * D * nc; i += kMotionThreads) tgt_s[i] = a.target[(size_t)r0 * D * nc + i];
    }
    constexpr int kU = kMotionMaxD * kMotionMaxKb / kMotionThreads;      // parameters per thread, at most
    float acc[kU][kMotionRows];
    int dd[kU], kk[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
        const int j = tid + u * kMotionThreads;
        dd[u] = j < P ? j / Kb : 0;
        kk[u] = j < P ? j - dd[u] * Kb : 0;
#pragma unroll
        for (int b = 0; b < kMotionRows; ++b) acc[u][b] = 0.0f;
    }
    for (int s0 = 0; s0 < T; s0 += kFitSlab) {
        const int ts = T - s0 < kFitSlab ? T - s0 : kFitSlab;
        __syncthreads();                                   // the previous slab is read
        for (int i = tid; i < ts * Kb; i += kMotionThreads) {
            const int t = i / Kb, k = i - t * Kb;
            phi_s[k * kLd + t] = a.phi[(size_t)s0 * Kb + i];
        }
        if (limited) for (int i = tid; i < ts * nc; i += kMotionThreads) gain_s[i] = a.gain[(size_t)s0 * nc + i];
        __syncthreads();
        for (int i = tid; i < kMotionRows * ts * D; i += kMotionThreads) {
            const int b = i / (ts * D), rem = i - b * ts * D, t = rem / D, d = rem - t * D;
            float g = 0.0f;
            if (b < nb) {
                g = a.grad_traj[((size_t)(r0 + b) * T + s0) * D + rem];
                if (limited) {
                    const float lo = a.limits[2 * d], hi = a.limits[2 * d + 1];
                    if (hi > lo) {                         // (the forward clamps this joint)
                        float q = 0.0f;
                        const float* th = th_s + (b * D + d) * kp;
                        for (int k = 0; k < Kb; ++k) q = __builtin_fmaf(phi_s[k * kLd + t], th[k], q);
                        for (int c = 0; c < nc; ++c) q = __builtin_fmaf(gain_s[t * nc + c], tgt_s[(b * D + d) * nc + c], q);
                        if (!(lo <= q && q <= hi)) g = 0.0f;
                    }
                }
            }
            g_s[b * kFitSlab * kMotionMaxD + rem] = g;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (tid + u * kMotionThreads >= P) continue;
            const float* pw = phi_s + kk[u] * kLd;
            const float* px = g_s + dd[u];
            for (int t = 0; t < ts; ++t) {
                const float w = pw[t];
#pragma unroll
                for (int b = 0; b < kMotionRows; ++b)
                    acc[u][b] = __builtin_fmaf(w, px[b * kFitSlab * kMotionMaxD + t * D], acc[u][b]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
        const int j = tid + u * kMotionThreads;
        if (j >= P) continue;
        const float sc = a.scale ? a.scale[j] : 1.0f;
        for (int b = 0; b < nb; ++b) a.grad_params[(size_t)(r0 + b) * P + j] = acc[u][b] * sc;
    }
}

// ------------------------------------------------------------------------------------------------ Adam, a row a problem
__global__ __launch_bounds__(kRowsAdamThreads) void k_rows_adam(const RowsAdamArgs a) {
    __shared__ float red[kRowsAdamThreads];
    constexpr int kE = kRowsAdamMaxN / kRowsAdamThreads;
    const int n = a.n, tid = threadIdx.x;
    const size_t row = blockIdx.x, at = row * (size_t)n;
    float x[kE], g[kE];
    int bad = 0;
    float ss = 0.0f;
#pragma unroll
    for (int j = 0; j < kE; ++j) {
        const int i = tid + j * kRowsAdamThreads;
        x[j] = 0.0f; g[j] = 0.0f;
        if (i < n) {
            x[j] = a.x[at + i]; g[j] = a.g[at + i];
            bad |= !latent_finite(g[j]);
            ss = __builtin_fmaf(g[j], g[j], ss);
        }
    }
    if (a.cost) {                                          // the parameters the cost was taken at, if they are the best so far
        const float c = a.cost[row];
        if (__syncthreads_or(c < a.best_cost[row])) {      // (uniform; every thread has read best_cost before thread 0 writes it)
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                const int i = tid + j * kRowsAdamThreads;
                if (i < n) a.best_x[at + i] = x[j];
            }
            if (tid == 0) a.best_cost[row] = c;
        }
    }
    if (__syncthreads_or(bad)) {                           // (uniform) a gradient that is not finite: the row stays as it is
        if (tid == 0) a.status[row] = 2;
        return;
    }
    red[tid] = ss;
    __syncthreads();
    for (int s = kRowsAdamThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    const float norm = sqrtf(red[0]);
    const float clip = a.max_norm > 0.0f ? fminf(1.0f, a.max_norm / norm) : 1.0f;
    const int step = a.t[row] + 1;
    const float bc1 = (float)(1.0 - pow((double)a.beta1, (double)step)), bc2 = (float)(1.0 - pow((double)a.beta2, (double)step));
    const float c1 = 1.0f - a.beta1, c2 = 1.0f - a.beta2;
#pragma unroll
    for (int j = 0; j < kE; ++j) {
        const int i = tid + j * kRowsAdamThreads;
        if (i < n) {
            const float gg = g[j] * clip;
            const float m = __builtin_fmaf(a.beta1, a.m[at + i], c1 * gg);
            const float v = __builtin_fmaf(a.beta2, a.v[at + i], (c2 * gg) * gg);
            a.m[at + i] = m; a.v[at + i] = v;
            a.x[at + i] = x[j] - (a.lr * (m / bc1)) / (sqrtf(v / bc2) + a.eps);
        }
    }
    if (tid == 0) { a.t[row] = step; a.status[row] = 0; }
}

}  // namespace

void launch_stroke_render_vjp(const RenderVjpArgs& a, long long rows, hipStream_t s) {
    const dim3 grid((unsigned)rows), block(kRenderThreads);
    const size_t lds = render_vjp_lds_bytes(a.f.T, a.f.H);
    const bool big = lds > 65536;                          // more than 64 KiB of dynamic LDS has to be allowed per kernel
    switch (a.f.ss) {
        case 1: if (big) allow_max_lds(k_stroke_render_vjp<1>); launch_kernel(k_stroke_render_vjp<1>, grid, block, lds, s, a); break;
        case 2: if (big) allow_max_lds(k_stroke_render_vjp<2>); launch_kernel(k_stroke_render_vjp<2>, grid, block, lds, s, a); break;
        case 4: if (big) allow_max_lds(k_stroke_render_vjp<4>); launch_kernel(k_stroke_render_vjp<4>, grid, block, lds, s, a); break;
        default: if (big) allow_max_lds(k_stroke_render_vjp<8>); launch_kernel(k_stroke_render_vjp<8>, grid, block, lds, s, a); break;
    }
}

void launch_motion_fk_vjp(const FkVjpArgs& a, hipStream_t s) {
    const long long tiles = (a.points + kRenderThreads - 1) / kRenderThreads;
    launch_kernel(k_motion_fk_vjp, dim3((unsigned)std::min<long long>(tiles, 1 << 20)), dim3(kRenderThreads), 0, s, a);
}

void launch_motion_eval_vjp(const MotionVjpArgs& a, hipStream_t s) {
    const long long tiles = (a.rows + kMotionRows - 1) / kMotionRows;
    launch_kernel(k_motion_eval_vjp, dim3((unsigned)tiles), dim3(kMotionThreads), 0, s, a);
}

void launch_rows_adam(const RowsAdamArgs& a, long long rows, hipStream_t s) {
    launch_kernel(k_rows_adam, dim3((unsigned)rows), dim3(kRowsAdamThreads), 0, s, a);
}

}  // namespace avae
