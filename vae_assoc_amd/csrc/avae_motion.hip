// Motion decoding kernels (avae_motion.h, include/avae.h): k_motion_eval, k_motion_moments, k_motion_fit.
#include "avae_device.h"
#include "avae_motion.h"

namespace avae {

namespace {

// Every operation below is the one written (a fused multiply-add only where __builtin_fmaf says so): tests/motion_reference.py
// restates them one by one.
#pragma clang fp contract(off)

struct Lds { float *phi, *gain, *th0, *th1, *tgt, *red; };

// The dynamic LDS of k_motion_eval / k_motion_moments (motion_lds_bytes): a slab's phi rows, its anchor gains, one or two theta
// tiles, the anchor targets of the workgroup's rows, the reduction buffer.
__device__ __forceinline__ Lds lds_layout(float* base, int D, int Kb, int T, int nc, bool two_tiles, int tgt_rows) {
    const int ts = motion_slab(D, Kb, T), kp = motion_pad(Kb), tile = kMotionRows * D * kp;
    Lds l;
    l.phi = base;
    l.gain = l.phi + ts * kp;
    l.th0 = l.gain + ts * nc;
    l.th1 = l.th0 + tile;
    l.tgt = l.th0 + tile * (two_tiles ? 2 : 1);
    const int used = (int)(l.tgt - base) + tgt_rows * D * nc;
    l.red = base + ((used + 1) & ~1);
    return l;
}

// A tile of up to kMotionRows consecutive parameter rows (n <= kMotionRows * 1024 floats at src) on its way from global memory
// to LDS: 16-byte loads over the aligned middle, thread tid the vectors tid, tid + 256, ...; the up to 3 floats in front of it
// go to threads 0..2 and the up to 3 behind it to threads 64..66, one scalar each.  Nothing outside [src, src + n) is read.
struct TileRegs { float4 v[kMotionRows]; float s; };

struct TileSplit { int head, nv, tail; };
__device__ __forceinline__ TileSplit tile_split(const float* src, int n) {
    TileSplit t;
    t.head = (int)((16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15) >> 2;
    t.head = t.head < n ? t.head : n;
    t.nv = (n - t.head) >> 2;
    t.tail = n - t.head - 4 * t.nv;
    return t;
}

__device__ __forceinline__ void tile_load(TileRegs& r, const float* src, int n) {
    const int tid = threadIdx.x;
    const TileSplit sp = tile_split(src, n);
    const float4* v = reinterpret_cast<const float4*>(src + sp.head);
#pragma unroll
    for (int u = 0; u < kMotionRows; ++u) {
        const int i = tid + u * kMotionThreads;
        if (i < sp.nv) r.v[u] = v[i];
    }
    if (tid < sp.head) r.s = src[tid];
    else if (tid >= 64 && tid - 64 < sp.tail) r.s = src[sp.head + 4 * sp.nv + tid - 64];
}

// Element e of the tile (row b = e / P, parameter j = e % P = d * Kb + k) -> theta = params * scale + shift at th[(b * D + d) * kp + k].
struct TilePos { int b, j, d, k; };
__device__ __forceinline__ TilePos tile_pos(int e, int P, int Kb) {
    TilePos p;
    p.b = e / P; p.j = e - p.b * P; p.d = p.j / Kb; p.k = p.j - p.d * Kb;
    return p;
}
__device__ __forceinline__ void tile_put(float* th, TilePos& p, float x, const MotionArgs& a, int P, int kp) {
    th[(p.b * a.D + p.d) * kp + p.k] = __builtin_fmaf(x, a.scale ? a.scale[p.j] : 1.0f, a.shift ? a.shift[p.j] : 0.0f);
    ++p.j;
    if (++p.k == a.Kb) { p.k = 0; ++p.d; }
    if (p.j == P) { p.j = 0; p.d = 0; p.k = 0; ++p.b; }
}

__device__ __forceinline__ void tile_store(const TileRegs& r, float* th, const float* src, int n, const MotionArgs& a, int P, int kp) {
    const int tid = threadIdx.x;
    const TileSplit sp = tile_split(src, n);
#pragma unroll
    for (int u = 0; u < kMotionRows; ++u) {
        const int i = tid + u * kMotionThreads;
        if (i < sp.nv) {
            TilePos p = tile_pos(sp.head + 4 * i, P, a.Kb);
            tile_put(th, p, r.v[u].x, a, P, kp);
            tile_put(th, p, r.v[u].y, a, P, kp);
            tile_put(th, p, r.v[u].z, a, P, kp);
            tile_put(th, p, r.v[u].w, a, P, kp);
        }
    }
    if (tid < sp.head) {
        TilePos p = tile_pos(tid, P, a.Kb);
        tile_put(th, p, r.s, a, P, kp);
    } else if (tid >= 64 && tid - 64 < sp.tail) {
        TilePos p = tile_pos(sp.head + 4 * sp.nv + tid - 64, P, a.Kb);
        tile_put(th, p, r.s, a, P, kp);
    }
}

// phi rows [s0, s0 + ts) (and their anchor gains) -> LDS, rows padded to kp floats
__device__ __forceinline__ void stage_slab(const Lds& l, const MotionArgs& a, int s0, int ts, int kp) {
    const float* src = a.phi + (size_t)s0 * a.Kb;
    for (int i = threadIdx.x; i < ts * a.Kb; i += kMotionThreads) {
        const int t = i / a.Kb, k = i - t * a.Kb;
        l.phi[t * kp + k] = src[i];
    }
    for (int i = threadIdx.x; i < ts * a.nc; i += kMotionThreads) l.gain[i] = a.gain[(size_t)s0 * a.nc + i];
}

// acc[b][j] = sum_k phi[tl[j]][k] * theta[b][d][k], k ascending, one fma each, from 0; th points at joint d of the tile's row 0
template <int NJ>
__device__ __forceinline__ void block_eval(const float* phi_s, const float* th, int Kb, int kp, int DK, const int (&tl)[kMotionJ],
                                           float (&acc)[kMotionRows][kMotionJ]) {
    const float* pp[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) pp[j] = phi_s + tl[j] * kp;
#pragma unroll
    for (int b = 0; b < kMotionRows; ++b)
#pragma unroll
        for (int j = 0; j < kMotionJ; ++j) acc[b][j] = 0.0f;
#pragma unroll 4
    for (int k = 0; k < Kb; ++k) {                 // (unrolled: 4 steps' LDS reads are in flight ahead of their fmas)
        float p[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) p[j] = pp[j][k];
#pragma unroll
        for (int b = 0; b < kMotionRows; ++b) {
            const float w = th[b * DK + k];
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[b][j] = __builtin_fmaf(p[j], w, acc[b][j]);
        }
    }
}

__device__ __forceinline__ void block_eval_n(int nj, const float* phi_s, const float* th, int Kb, int kp, int DK,
                                             const int (&tl)[kMotionJ], float (&acc)[kMotionRows][kMotionJ]) {
    switch (nj) {                                   // (uniform over the workgroup)
        case 1: block_eval<1>(phi_s, th, Kb, kp, DK, tl, acc); break;
        case 2: block_eval<2>(phi_s, th, Kb, kp, DK, tl, acc); break;
        case 3: block_eval<3>(phi_s, th, Kb, kp, DK, tl, acc); break;
        default: block_eval<4>(phi_s, th, Kb, kp, DK, tl, acc); break;
    }
}

// the anchor terms in index order, then the clamp by comparison (a NaN stays NaN and is not counted)
__device__ __forceinline__ float finish(float q, const float* g, const float* tg, int nc, bool clamp, float lo, float hi, int& sat) {
    for (int c = 0; c < nc; ++c) q = __builtin_fmaf(g[c], tg[c], q);
    if (clamp) {
        if (q > hi) { q = hi; ++sat; }
        if (q < lo) { q = lo; ++sat; }
    }
    return q;
}

struct Owner { bool active; int d, tq, TQ; };
__device__ __forceinline__ Owner owner_of(int D) {
    Owner o;
    o.TQ = motion_tq(D);
    o.active = (int)threadIdx.x < o.TQ * D;
    o.d = o.active ? (int)threadIdx.x % D : 0;
    o.tq = o.active ? (int)threadIdx.x / D : 0;
    return o;
}

// red[tid] over the TQ threads of a joint, a fixed tree: afterwards the joint's value is at red[d].  All threads call it.
template <typename V, typename F>
__device__ __forceinline__ void joint_tree(V* red, const Owner& o, int D, F&& combine) {
    __syncthreads();
    for (int s = kMotionThreads / 2; s > 0; s >>= 1) {
        if (o.active && o.tq < s && o.tq + s < o.TQ) red[threadIdx.x] = combine(red[threadIdx.x], red[threadIdx.x + s * D]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(kMotionThreads) void k_motion_eval(const MotionArgs a) {
    extern __shared__ __align__(16) float motion_smem[];
    const int D = a.D, Kb = a.Kb, T = a.T, nc = a.nc, P = D * Kb, kp = motion_pad(Kb), DK = D * kp, TS = motion_slab(D, Kb, T);
    const int tid = threadIdx.x;
    const Owner o = owner_of(D);
    const long long r0 = (long long)blockIdx.x * kMotionRows;
    const int nb = (int)(a.rows - r0 < kMotionRows ? a.rows - r0 : kMotionRows);
    const bool by_params = a.ref_params != nullptr, has_ref = by_params || a.ref_traj != nullptr;
    const Lds l = lds_layout(motion_smem, D, Kb, T, nc, by_params, kMotionRows);

    {
        TileRegs rg;
        const float* src = a.params + (size_t)r0 * P;
        tile_load(rg, src, nb * P);
        tile_store(rg, l.th0, src, nb * P, a, P, kp);
        if (by_params) {
            src = a.ref_params + (size_t)r0 * P;
            tile_load(rg, src, nb * P);
            tile_store(rg, l.th1, src, nb * P, a, P, kp);
        }
        for (int i = tid; i < nb * D * nc; i += kMotionThreads) l.tgt[i] = a.target[(size_t)r0 * D * nc + i];
    }
    const float lo = a.limits ? a.limits[2 * o.d] : 0.0f, hi = a.limits ? a.limits[2 * o.d + 1] : 0.0f;
    const bool clamp = a.limits != nullptr && hi > lo;

    float ssq[kMotionRows], mx[kMotionRows];
    int sat[kMotionRows];
#pragma unroll
    for (int b = 0; b < kMotionRows; ++b) { ssq[b] = 0.0f; mx[b] = 0.0f; sat[b] = 0; }

    for (int s0 = 0; s0 < T; s0 += TS) {
        const int ts = T - s0 < TS ? T - s0 : TS;
        __syncthreads();                                   // the previous slab is read; the first time: nothing to wait for
        stage_slab(l, a, s0, ts, kp);
        __syncthreads();
        if (!o.active) continue;
        const int nj = (ts + o.TQ - 1) / o.TQ;
        int tl[kMotionJ];
        bool ok[kMotionJ];
#pragma unroll
        for (int j = 0; j < kMotionJ; ++j) {
            const int t = o.tq + j * o.TQ;
            ok[j] = t < ts;
            tl[j] = ok[j] ? t : 0;
        }
        float acc[kMotionRows][kMotionJ], accr[kMotionRows][kMotionJ];
        block_eval_n(nj, l.phi, l.th0 + o.d * kp, Kb, kp, DK, tl, acc);
        if (by_params) block_eval_n(nj, l.phi, l.th1 + o.d * kp, Kb, kp, DK, tl, accr);
#pragma unroll
        for (int b = 0; b < kMotionRows; ++b) {
            if (b >= nb) continue;
#pragma unroll
            for (int j = 0; j < kMotionJ; ++j) {
                if (!ok[j]) continue;
                const size_t at = ((size_t)(r0 + b) * T + s0 + tl[j]) * D + o.d;
                const float q = finish(acc[b][j], l.gain + tl[j] * nc, l.tgt + (b * D + o.d) * nc, nc, clamp, lo, hi, sat[b]);
                if (a.traj) a.traj[at] = q;
                if (has_ref) {
                    int unused = 0;
                    const float qr = by_params ? finish(accr[b][j], nullptr, nullptr, 0, clamp, lo, hi, unused) : a.ref_traj[at];
                    const float e = q - qr, ae = fabsf(e);
                    ssq[b] = __builtin_fmaf(e, e, ssq[b]);
                    if (ae > mx[b] || ae != ae) mx[b] = ae;
                }
            }
        }
    }

    // the sums over t of a (row, joint): the threads' own values (t ascending), then the tree over the joint's threads
    int* redi = reinterpret_cast<int*>(l.red);
    if (a.rmse) {
        __syncthreads();
        for (int b = 0; b < kMotionRows; ++b) l.red[b * kMotionThreads + tid] = ssq[b];
        for (int b = 0; b < kMotionRows; ++b)
            joint_tree(l.red + b * kMotionThreads, o, D, [](float x, float y) { return x + y; });
        if (o.active && o.tq == 0)
            for (int b = 0; b < nb; ++b) a.rmse[(size_t)(r0 + b) * D + o.d] = sqrtf(l.red[b * kMotionThreads + o.d] / (float)T);
    }
    if (a.maxabs) {
        __syncthreads();
        for (int b = 0; b < kMotionRows; ++b) l.red[b * kMotionThreads + tid] = mx[b];
        for (int b = 0; b < kMotionRows; ++b)
            joint_tree(l.red + b * kMotionThreads, o, D, [](float x, float y) { return (y > x || y != y) ? y : x; });
        if (o.active && o.tq == 0)
            for (int b = 0; b < nb; ++b) a.maxabs[(size_t)(r0 + b) * D + o.d] = l.red[b * kMotionThreads + o.d];
    }
    if (a.saturated) {
        __syncthreads();
        for (int b = 0; b < kMotionRows; ++b) redi[b * kMotionThreads + tid] = sat[b];
        for (int b = 0; b < kMotionRows; ++b)
            joint_tree(redi + b * kMotionThreads, o, D, [](int x, int y) { return x + y; });
        if (o.active && o.tq == 0)
            for (int b = 0; b < nb; ++b) a.saturated[(size_t)(r0 + b) * D + o.d] = redi[b * kMotionThreads + o.d];
    }
}

__global__ __launch_bounds__(kMotionThreads) void k_motion_moments(const MotionArgs a) {
    extern __shared__ __align__(16) float motion_smem[];
    const int D = a.D, Kb = a.Kb, T = a.T, nc = a.nc, S = a.S, P = D * Kb, kp = motion_pad(Kb), DK = D * kp, TS = motion_slab(D, Kb, T);
    const int tid = threadIdx.x;
    const Owner o = owner_of(D);
    const size_t r = blockIdx.x;
    const Lds l = lds_layout(motion_smem, D, Kb, T, nc, true, 1);
    const float* src = a.params + r * (size_t)S * P;
    const int n_tiles = (S + kMotionRows - 1) / kMotionRows;

    for (int i = tid; i < D * nc; i += kMotionThreads) l.tgt[i] = a.target[r * D * nc + i];
    const float lo = a.limits ? a.limits[2 * o.d] : 0.0f, hi = a.limits ? a.limits[2 * o.d + 1] : 0.0f;
    const bool clamp = a.limits != nullptr && hi > lo;
    long long sat = 0;

    for (int s0 = 0; s0 < T; s0 += TS) {
        const int ts = T - s0 < TS ? T - s0 : TS;
        TileRegs rg;
        {
            const int n0 = (S < kMotionRows ? S : kMotionRows) * P;
            tile_load(rg, src, n0);
            __syncthreads();                               // the previous slab's last tile and phi rows are read
            stage_slab(l, a, s0, ts, kp);
            tile_store(rg, l.th0, src, n0, a, P, kp);
        }
        __syncthreads();
        const int nj = (ts + o.TQ - 1) / o.TQ;
        int tl[kMotionJ];
        bool ok[kMotionJ];
        float mean[kMotionJ], m2[kMotionJ];
#pragma unroll
        for (int j = 0; j < kMotionJ; ++j) {
            const int t = o.tq + j * o.TQ;
            ok[j] = o.active && t < ts;
            tl[j] = ok[j] ? t : 0;
            mean[j] = 0.0f; m2[j] = 0.0f;
        }
        for (int i = 0; i < n_tiles; ++i) {
            const int left = S - (i + 1) * kMotionRows;
            const int n_next = (left < 0 ? 0 : left < kMotionRows ? left : kMotionRows) * P;
            const float* next = src + (size_t)(i + 1) * kMotionRows * P;
            if (n_next) tile_load(rg, next, n_next);       // in flight while this tile is evaluated
            const int nb = S - i * kMotionRows < kMotionRows ? S - i * kMotionRows : kMotionRows;
            if (o.active) {
                float acc[kMotionRows][kMotionJ];
                block_eval_n(nj, l.phi, ((i & 1) ? l.th1 : l.th0) + o.d * kp, Kb, kp, DK, tl, acc);
#pragma unroll
                for (int b = 0; b < kMotionRows; ++b) {
                    if (b >= nb) continue;
                    const float count = (float)(i * kMotionRows + b + 1);
#pragma unroll
                    for (int j = 0; j < kMotionJ; ++j) {
                        if (!ok[j]) continue;
                        int hit = 0;
                        const float q = finish(acc[b][j], l.gain + tl[j] * nc, l.tgt + o.d * nc, nc, clamp, lo, hi, hit);
                        sat += hit;
                        const float delta = q - mean[j];
                        mean[j] = mean[j] + delta / count;
                        m2[j] = __builtin_fmaf(delta, q - mean[j], m2[j]);
                    }
                }
            }
            if (n_next) tile_store(rg, (i & 1) ? l.th0 : l.th1, next, n_next, a, P, kp);
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < kMotionJ; ++j) {
            if (!ok[j]) continue;
            const size_t at = (r * T + s0 + tl[j]) * D + o.d;
            a.traj[at] = mean[j];
            if (a.var) a.var[at] = m2[j] / (float)S;
        }
    }
    if (a.sat_frac) {
        long long* red = reinterpret_cast<long long*>(l.red);
        __syncthreads();
        red[tid] = sat;
        joint_tree(red, o, D, [](long long x, long long y) { return x + y; });
        if (o.active && o.tq == 0) a.sat_frac[r * D + o.d] = (float)((double)red[o.d] / ((double)S * (double)T));
    }
}

// theta[r][d][k] = sum_t pinv[k][t] * traj[r][t][d], t ascending, one fma each, from 0; params = (theta - shift) / scale
__global__ __launch_bounds__(kMotionThreads) void k_motion_fit(const MotionFitArgs a) {
    constexpr int kLd = kFitSlab + 1;
    __shared__ float pinv_s[kMotionMaxKb * kLd];
    __shared__ float traj_s[kMotionRows * kFitSlab * kMotionMaxD];
    const int D = a.D, Kb = a.Kb, T = a.T, P = D * Kb, tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * kMotionRows;
    const int nb = (int)(a.rows - r0 < kMotionRows ? a.rows - r0 : kMotionRows);
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
        __syncthreads();
        for (int i = tid; i < Kb * ts; i += kMotionThreads) {
            const int k = i / ts, t = i - k * ts;
            pinv_s[k * kLd + t] = a.pinv[(size_t)k * T + s0 + t];
        }
        for (int b = 0; b < kMotionRows; ++b)
            for (int i = tid; i < ts * D; i += kMotionThreads)
                traj_s[b * kFitSlab * kMotionMaxD + i] = b < nb ? a.traj[((size_t)(r0 + b) * T + s0) * D + i] : 0.0f;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (tid + u * kMotionThreads >= P) continue;
            const float* pw = pinv_s + kk[u] * kLd;
            const float* px = traj_s + dd[u];
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
        const float sc = a.scale ? a.scale[j] : 1.0f, sh = a.shift ? a.shift[j] : 0.0f;
        for (int b = 0; b < nb; ++b) a.params[(size_t)(r0 + b) * P + j] = (acc[u][b] - sh) / sc;
    }
}

}  // namespace

void launch_motion_eval(const MotionArgs& a, hipStream_t s) {
    const long long tiles = (a.rows + kMotionRows - 1) / kMotionRows;
    launch_kernel(k_motion_eval, dim3((unsigned)tiles), dim3(kMotionThreads), motion_lds_bytes(a.D, a.Kb, a.T, a.nc, false, a.ref_params != nullptr), s, a);
}

void launch_motion_moments(const MotionArgs& a, hipStream_t s) {
    launch_kernel(k_motion_moments, dim3((unsigned)a.rows), dim3(kMotionThreads), motion_lds_bytes(a.D, a.Kb, a.T, a.nc, true, false), s, a);
}

void launch_motion_fit(const MotionFitArgs& a, hipStream_t s) {
    const long long tiles = (a.rows + kMotionRows - 1) / kMotionRows;
    launch_kernel(k_motion_fit, dim3((unsigned)tiles), dim3(kMotionThreads), 0, s, a);
}

}  // namespace avae
