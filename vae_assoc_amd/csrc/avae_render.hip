// Pen-path kinematics and stroke rendering kernels (avae_render.h, include/avae.h): k_motion_fk, k_stroke_render.
#include "avae_device.h"
#include "avae_render.h"

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
enum { kSum = 0, kMin = 1, kMax = 2 };

// THE TREE over the workgroup's 256 values of each of K columns (column k combined by op[k]); every thread gets the results.
template <int K>
__device__ __forceinline__ void block_tree(float* red, float (&v)[K], const int (&op)[K]) {
    const int tid = threadIdx.x;
    __syncthreads();                                       // the previous tree's results are read
#pragma unroll
    for (int k = 0; k < K; ++k) red[k * kRenderThreads + tid] = v[k];
    __syncthreads();
    for (int s = kRenderThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float x = red[k * kRenderThreads + tid], y = red[k * kRenderThreads + tid + s];
                red[k * kRenderThreads + tid] = op[k] == kSum ? x + y : op[k] == kMin ? fminf(x, y) : fmaxf(x, y);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = red[k * kRenderThreads];
}

// the squared distance of (u, v) to one segment record, as avae_render.h writes it
__device__ __forceinline__ float seg_dist2(float u, float py, float pydy, const float4& g, float inv) {
    const float px = u - g.x;
    float t = __builtin_fmaf(px, g.z, pydy) * inv;
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    const float ex = __builtin_fmaf(-t, g.z, px), ey = __builtin_fmaf(-t, g.w, py);
    return __builtin_fmaf(ey, ey, ex * ex);
}

struct Frame { float u0, v0, delta, r; };

// One pass of step 5: sub-row `it` of the inked list (ss samples) -> its coverage sum.
template <int SS>
__device__ __forceinline__ float subrow_sum(int it, const unsigned short* list, const float4* seg, const float* inv, int nseg, int H,
                                            const Frame& f) {
    const int pix = list[it / SS], sa = it % SS, i = pix / H, j = pix - i * H;
    const float v = __builtin_fmaf(-((float)(i * SS + sa) + 0.5f), f.delta, f.v0);
    float u[SS], m[SS];
#pragma unroll
    for (int b = 0; b < SS; ++b) {
        u[b] = __builtin_fmaf((float)(j * SS + b) + 0.5f, f.delta, f.u0);
        m[b] = __builtin_inff();
    }
    for (int s = 0; s < nseg; ++s) {
        const float4 g = seg[s];
        const float iv = inv[s], py = v - g.y, pydy = py * g.w;
#pragma unroll
        for (int b = 0; b < SS; ++b) m[b] = fminf(m[b], seg_dist2(u[b], py, pydy, g, iv));
    }
    float sum = 0.0f;
#pragma unroll
    for (int b = 0; b < SS; ++b) {
        const float x = 0.5f + (f.r - sqrtf(m[b])) / f.delta;
        const float cov = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;
        sum = b == 0 ? cov : sum + cov;
    }
    return sum;
}

template <int SS>
__global__ __launch_bounds__(kRenderThreads) void k_stroke_render(const RenderArgs a) {
    extern __shared__ __align__(16) float render_smem[];
    const int T = a.T, H = a.H, npx = H * H, nseg = T > 1 ? T - 1 : 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row = blockIdx.x;
    const RenderLds l = render_lds(T, H);
    float4* seg = reinterpret_cast<float4*>(render_smem + l.seg);
    float *inv = render_smem + l.inv, *cu = render_smem + l.cu, *cv = render_smem + l.cv, *img = render_smem + l.img;
    float *red = render_smem + l.red, *rows_s = render_smem + l.rows;
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(render_smem + l.mask);
    int* base = reinterpret_cast<int*>(render_smem + l.base);
    unsigned short* list = reinterpret_cast<unsigned short*>(render_smem + l.list);
    constexpr int kPts = kRenderMaxT / kRenderThreads;

    // 1. the mean
    const float* path = a.path + row * (size_t)T * 3;
    float px[kPts], py[kPts], pz[kPts];
    float sum[3] = {0.0f, 0.0f, 0.0f};
    int bad = 0;
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        const int t = tid + j * kRenderThreads;
        px[j] = py[j] = pz[j] = 0.0f;
        if (t < T) {
            px[j] = path[3 * t]; py[j] = path[3 * t + 1]; pz[j] = path[3 * t + 2];
            bad |= !(latent_finite(px[j]) && latent_finite(py[j]) && latent_finite(pz[j]));
            sum[0] = sum[0] + px[j]; sum[1] = sum[1] + py[j]; sum[2] = sum[2] + pz[j];
        }
    }
    if (__syncthreads_or(bad)) {                           // (uniform) a non-finite row: NaN everywhere, nothing else
        const float nan = __builtin_nanf("");
        if (a.image) for (int p = tid; p < npx; p += kRenderThreads) a.image[row * npx + p] = nan;
        if (a.window && tid < 3) a.window[row * 3 + tid] = nan;
        if (a.img_l2 && tid == 0) a.img_l2[row] = nan;
        if (a.height_l2 && tid == 0) a.height_l2[row] = nan;
        return;
    }
    {
        const int op[3] = {kSum, kSum, kSum};
        block_tree<3>(red, sum, op);
    }
    const float mx = sum[0] / (float)T, my = sum[1] / (float)T, mz = sum[2] / (float)T;

    // 2. projection, ink box, height
    const float* pl = a.plane;
    const float u0 = pl[0], u1 = pl[1], u2 = pl[2], v0 = pl[3], v1 = pl[4], v2 = pl[5], n0 = pl[6], n1 = pl[7], n2 = pl[8];
    const float hgt = a.height_l2 ? a.height[row] : 0.0f;
    float box[5] = {__builtin_inff(), -__builtin_inff(), __builtin_inff(), -__builtin_inff(), 0.0f};
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        const int t = tid + j * kRenderThreads;
        if (t < T) {
            const float dx = px[j] - mx, dy = py[j] - my, dz = pz[j] - mz;
            const float c0 = __builtin_fmaf(u2, dz, __builtin_fmaf(u1, dy, u0 * dx));
            const float c1 = __builtin_fmaf(v2, dz, __builtin_fmaf(v1, dy, v0 * dx));
            cu[t] = c0; cv[t] = c1;
            box[0] = fminf(box[0], c0); box[1] = fmaxf(box[1], c0); box[2] = fminf(box[2], c1); box[3] = fmaxf(box[3], c1);
            const float e = __builtin_fmaf(n2, pz[j], __builtin_fmaf(n1, py[j], n0 * px[j])) - hgt;
            box[4] = __builtin_fmaf(e, e, box[4]);
        }
    }
    {
        const int op[5] = {kMin, kMax, kMin, kMax, kSum};
        block_tree<5>(red, box, op);                       // (its barriers also publish cu / cv)
    }
    const float r = a.half_width;
    const float lo_u = box[0] - r, hi_u = box[1] + r, lo_v = box[2] - r, hi_v = box[3] + r;
    const float ctr_u = (lo_u + hi_u) * 0.5f, ctr_v = (lo_v + hi_v) * 0.5f;
    const float L = fmaxf(hi_u - lo_u, hi_v - lo_v), W = (1.0f + a.margin) * L;
    Frame f;
    f.delta = W / (float)(H * SS);
    f.u0 = ctr_u - 0.5f * W;
    f.v0 = ctr_v + 0.5f * W;
    f.r = r;
    if (tid == 0) {
        if (a.window) { a.window[row * 3] = ctr_u; a.window[row * 3 + 1] = ctr_v; a.window[row * 3 + 2] = W; }
        if (a.height_l2) a.height_l2[row] = sqrtf(box[4]);
    }
    if (!a.image && !a.img_l2) return;                     // (uniform)

    // 3. segment records; the image starts as +0
    for (int s = tid; s < nseg; s += kRenderThreads) {
        const int s1 = s + 1 < T ? s + 1 : T - 1;
        const float ax = cu[s], ay = cv[s], dx = cu[s1] - ax, dy = cv[s1] - ay;
        const float len2 = __builtin_fmaf(dy, dy, dx * dx);
        seg[s] = make_float4(ax, ay, dx, dy);
        inv[s] = len2 >= kRenderMinLen2 ? 1.0f / len2 : 0.0f;
    }
    for (int p = tid; p < npx; p += kRenderThreads) img[p] = 0.0f;
    __syncthreads();

    // 4. which pixels can hold ink
    const int nchunk = (npx + 63) >> 6;
    {
        const float thr = ((r + 0.5f * f.delta) + kRenderHalfDiag * (float)SS * f.delta) * kRenderCullSafety, thr2 = thr * thr;
        const float half = 0.5f * (float)SS;
        for (int k0 = wave; k0 < nchunk; k0 += 8) {
            float cu_[2], cv_[2], m[2];
            bool in[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int p = (k0 + 4 * e) * 64 + lane, i = p / H, j = p - i * H;
                cu_[e] = __builtin_fmaf((float)(j * SS) + half, f.delta, f.u0);
                cv_[e] = __builtin_fmaf(-((float)(i * SS) + half), f.delta, f.v0);
                const float bx = fmaxf(fmaxf(box[0] - cu_[e], cu_[e] - box[1]), 0.0f);
                const float by = fmaxf(fmaxf(box[2] - cv_[e], cv_[e] - box[3]), 0.0f);
                in[e] = p < npx && __builtin_fmaf(by, by, bx * bx) < thr2;
                m[e] = __builtin_inff();
            }
            if (in[0] || in[1]) {
                for (int s = 0; s < nseg; ++s) {
                    const float4 g = seg[s];
                    const float iv = inv[s];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const float py_ = cv_[e] - g.y;
                        m[e] = fminf(m[e], seg_dist2(cu_[e], py_, py_ * g.w, g, iv));
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const unsigned long long bits = __ballot(in[e] && m[e] < thr2);
                if (lane == 0 && k0 + 4 * e < nchunk) mask[k0 + 4 * e] = bits;
            }
        }
    }
    __syncthreads();
    if (tid <= nchunk) {
        int n = 0;
        for (int k = 0; k < tid; ++k) n += __popcll(mask[k]);
        base[tid] = n;
    }
    __syncthreads();
    for (int k = wave; k < nchunk; k += 4) {
        const unsigned long long bits = mask[k];
        if ((bits >> lane) & 1ull) list[base[k] + __popcll(bits & ((1ull << lane) - 1ull))] = (unsigned short)(k * 64 + lane);
    }
    __syncthreads();
    const int items = base[nchunk] * SS;

    // 5. the inked pixels, a sub-row per thread
    constexpr float kInvArea = 1.0f / (float)(SS * SS);
    for (int it0 = 0; it0 < items; it0 += kRenderThreads) {
        const int it = it0 + tid;
        if (it < items) rows_s[tid] = subrow_sum<SS>(it, list, seg, inv, nseg, H, f);
        __syncthreads();
        if (tid < kRenderThreads / SS && it0 + tid * SS < items) {
            float s = rows_s[tid * SS];
#pragma unroll
            for (int k = 1; k < SS; ++k) s = s + rows_s[tid * SS + k];
            img[list[it0 / SS + tid]] = s * kInvArea;
        }
        __syncthreads();
    }

    // 6. out
    float e2[1] = {0.0f};
    for (int p = tid; p < npx; p += kRenderThreads) {
        const float x = img[p];
        if (a.image) a.image[row * npx + p] = x;
        if (a.img_l2) {
            const float e = x - a.target[row * npx + p];
            e2[0] = __builtin_fmaf(e, e, e2[0]);
        }
    }
    if (a.img_l2) {
        const int op[1] = {kSum};
        block_tree<1>(red, e2, op);
        if (tid == 0) a.img_l2[row] = sqrtf(e2[0]);
    }
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
