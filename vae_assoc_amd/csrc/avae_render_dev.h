// The device code of the stroke renderer that k_stroke_render (avae_render.hip) and k_stroke_render_vjp (avae_grad.hip) share
// (avae_render.h writes the steps down; DESIGN.md sections 24 and 31): THE TREE, the distance to a segment record, one pass of step
// 5 and render_row, the whole forward pass of one row.  Both kernels call the same render_row, so the forward outputs the reverse
// pass writes on request are the forward kernel's bits.  Device code only: include it from a .hip file, once.
#pragma once
#include "avae_device.h"
#include "avae_render.h"

namespace avae {

namespace {

// Every operation below is the one written (a fused multiply-add only where __builtin_fmaf says so): tests/render_reference.py
// restates them one by one.
#pragma clang fp contract(off)

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

// What render_row leaves behind for a caller that goes on with the row: in LDS the segment records, cu / cv, the image and the inked
// list (`items` sub-rows); here the frame, the exact ink box (min u, max u, min v, max v) and the two distances.
struct RenderRow {
    bool bad;                 // (uniform) a non-finite coordinate: the row's forward outputs are written as NaN, nothing else is valid
    bool drawn;               // (uniform) steps 3 to 6 ran
    Frame f;
    float box[4];
    bool longer_u;            // longer_u: hi_u - lo_u >= hi_v - lo_v (the side that sets the window; u wins a tie)
    float W, img_l2, height_l2;
    int items;
};

// The forward pass of row blockIdx.x: steps 1 to 6 of avae_render.h.  `draw`: steps 3 to 6 are wanted; `want_l2` / `want_h`: the
// two distances are computed (a.target / a.height are read) and stored where a.img_l2 / a.height_l2 are given.  All uniform.
template <int SS>
__device__ __forceinline__ RenderRow render_row(const RenderArgs& a, float* render_smem, const RenderLds& l, bool draw, bool want_l2,
                                                bool want_h) {
    const int T = a.T, H = a.H, npx = H * H, nseg = T > 1 ? T - 1 : 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row = blockIdx.x;
    float4* seg = reinterpret_cast<float4*>(render_smem + l.seg);
    float *inv = render_smem + l.inv, *cu = render_smem + l.cu, *cv = render_smem + l.cv, *img = render_smem + l.img;
    float *red = render_smem + l.red, *rows_s = render_smem + l.rows;
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(render_smem + l.mask);
    int* base = reinterpret_cast<int*>(render_smem + l.base);
    unsigned short* list = reinterpret_cast<unsigned short*>(render_smem + l.list);
    constexpr int kPts = kRenderMaxT / kRenderThreads;
    RenderRow out;
    out.bad = false; out.drawn = false; out.items = 0; out.img_l2 = 0.0f; out.height_l2 = 0.0f;

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
        out.bad = true;
        return out;
    }
    {
        const int op[3] = {kSum, kSum, kSum};
        block_tree<3>(red, sum, op);
    }
    const float mx = sum[0] / (float)T, my = sum[1] / (float)T, mz = sum[2] / (float)T;

    // 2. projection, ink box, height
    const float* pl = a.plane;
    const float u0 = pl[0], u1 = pl[1], u2 = pl[2], v0 = pl[3], v1 = pl[4], v2 = pl[5], n0 = pl[6], n1 = pl[7], n2 = pl[8];
    const float hgt = want_h ? a.height[row] : 0.0f;
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
    out.f = f; out.W = W; out.longer_u = hi_u - lo_u >= hi_v - lo_v;
    out.box[0] = box[0]; out.box[1] = box[1]; out.box[2] = box[2]; out.box[3] = box[3];
    out.height_l2 = sqrtf(box[4]);
    if (tid == 0) {
        if (a.window) { a.window[row * 3] = ctr_u; a.window[row * 3 + 1] = ctr_v; a.window[row * 3 + 2] = W; }
        if (a.height_l2) a.height_l2[row] = out.height_l2;
    }
    if (!draw) return out;                                 // (uniform)
    out.drawn = true;

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
    out.items = items;

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
        if (want_l2) {
            const float e = x - a.target[row * npx + p];
            e2[0] = __builtin_fmaf(e, e, e2[0]);
        }
    }
    if (want_l2) {
        const int op[1] = {kSum};
        block_tree<1>(red, e2, op);
        out.img_l2 = sqrtf(e2[0]);
        if (tid == 0 && a.img_l2) a.img_l2[row] = out.img_l2;
    }
    return out;
}

}  // namespace

}  // namespace avae
