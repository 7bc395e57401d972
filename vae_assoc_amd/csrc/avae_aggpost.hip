// Aggregate-posterior log-density kernels of libavae (gfx950): log q_agg(z) = log (1/G') sum_g N(z; mu_g, diag exp(lv_g)) and its
// per-dimension marginals as one streamed log-sum-exp (avae_agg_logpdf in include/avae.h; the plan, the scratch and the launch
// shapes: avae_aggpost.h).  The rows x gallery_rows x n_z tensor of exponents lives in registers only.
#include "avae_device.h"
#include "avae_aggpost.h"

namespace avae {

namespace {

// Every float operation below is the one written: the value of a query must not depend on which lane, wave or tile formed it, so
// nothing is left to the contraction pass.
#pragma clang fp contract(off)

constexpr float kLog2e = 1.44269504088896340736f;

// exp(x) for x <= 0 (or -Inf, NaN) inside the sums: the hardware exponential on a pre-scaled argument.  exp2(-Inf) = +0, NaN stays.
__device__ __forceinline__ float agg_exp(float x) { return __builtin_amdgcn_exp2f(x * kLog2e); }

// THE exponent of one (query, gallery row, dimension): l = -0.5f * fmaf(d*d, iv, lv) with the -0.5f folded into the staged
// hiv = -0.5f * iv and hlv = -0.5f * lv (an exact scaling by a power of two on both sides of the one rounding).
__device__ __forceinline__ float agg_term(float z, float mu, float hiv, float hlv) {
    const float d = z - mu;
    return __builtin_fmaf(d * d, hiv, hlv);
}

// Rows of a block that do not count -- past the end of the gallery (i >= valid) or the query's excluded row (i == off) -- are
// selected away: their exponent becomes -Inf whatever was computed from them.
__device__ __forceinline__ void agg_select(float (&l)[kAggBlock], int valid, int off) {
#pragma unroll
    for (int i = 0; i < kAggBlock; ++i)
        if (i >= valid || i == off) l[i] = -__builtin_inff();
}

// One block of 8 exponents joins a running (max m, sum s of exp(l - m)): the max of the 8 against m (fmaxf: a NaN never becomes
// the max), ONE rescale of s, the 8 exponentials added in row order.  While everything is -Inf the shift is 0 instead, so that
// (-Inf) - (-Inf) never forms: the terms are exp(-Inf) = 0 and a NaN exponent still makes the sum NaN.
__device__ __forceinline__ void agg_block(const float (&l)[kAggBlock], float& m, float& s) {
    float bm = m;
#pragma unroll
    for (int i = 0; i < kAggBlock; ++i) bm = __builtin_fmaxf(bm, l[i]);
    const float shift = bm == -__builtin_inff() ? 0.0f : bm;
    float acc = s * agg_exp(m - shift);
#pragma unroll
    for (int i = 0; i < kAggBlock; ++i) acc = acc + agg_exp(l[i] - shift);
    m = bm;
    s = acc;
}

// grid (query tiles, gallery slices), kAggThreads threads: lane = query of the tile, wave w = the marginals' columns w, w + 8, ...
// and the joint's block w of every gallery tile.
template <bool MARG, bool JOINT>
__global__ void __launch_bounds__(kAggThreads) k_agg_logpdf(AggArgs a) {
    constexpr int TQ = kAggQueryTile, TG = kAggGalleryTile, LQ = kAggQueryLd, LG = kAggGalleryLd, BL = kAggBlock, NW = kAggWaves;
    constexpr int PER = TG * kAggMaxNz / kAggThreads;              // staged elements per thread and tile, at most (8)
    constexpr int NC = kAggMaxNz / NW;                             // columns of one wave, at most (8)
    static_assert(TQ == TG && PER * kAggThreads == TG * kAggMaxNz && TQ == 64, "one staging pattern for both sides; lane = query");
    extern __shared__ __attribute__((aligned(16))) unsigned char agg_lds[];
    const int nz = a.nz;
    float* gm = reinterpret_cast<float*>(agg_lds);                 // [nz][LG] mu
    float* gh = gm + nz * LG;                                      // [nz][LG] -0.5 * expf(-lv)
    float* gl = gh + nz * LG;                                      // [nz][LG] -0.5 * lv
    float2* jp = reinterpret_cast<float2*>(gl + nz * LG);          // [NW][TQ] the joint's (m, s) per block position
    float* zi = reinterpret_cast<float*>(jp + NW * TQ);            // [nz][LQ]
    static_assert(kAggGalleryLd % 4 == 0 && kAggBlock % 4 == 0, "the 16-byte reads of four gallery rows are aligned for every n_z");
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long q0 = (long long)blockIdx.x * TQ;
    const int nq = (int)min((long long)TQ, a.rows - q0);           // valid queries of the tile (>= 1)
    const long long g_lo = (long long)blockIdx.y * a.slice_rows;
    const long long g_hi = min((long long)a.gallery_rows, g_lo + a.slice_rows);
    const int n_tiles = (int)((g_hi - g_lo + TG - 1) / TG);       // >= 1: no slice is empty
    const int n_el = TG * nz;

    int row_of[PER], dim_of[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int e = tid + r * kAggThreads;
        row_of[r] = e / nz; dim_of[r] = e - row_of[r] * nz;
    }
    // the query tile: resident for the whole slice; rows past the end are zeros (finite arithmetic, results never written)
    {
        const float* zq = a.z + q0 * nz;
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int e = tid + r * kAggThreads;
            if (e < n_el) zi[dim_of[r] * LQ + row_of[r]] = e < nq * nz ? zq[e] : 0.0f;
        }
    }
    int ex = -1;                                                   // the query's excluded gallery row, -1: none
    if (a.exclude && lane < nq) {
        ex = a.exclude[q0 + lane];
        if (ex < 0 || ex >= a.gallery_rows) ex = -1;
    }
    float pm[PER], pl[PER];                                        // the next gallery tile on its way from memory
    auto fetch = [&](int t) {
        const long long g0 = g_lo + (long long)t * TG;
        const int ng = (int)min((long long)TG, g_hi - g0);
        const float* m = a.g_mu + g0 * nz;
        const float* l = a.g_lv + g0 * nz;
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int e = tid + r * kAggThreads;
            const bool in = e < ng * nz;
            pm[r] = in ? m[e] : 0.0f;
            pl[r] = in ? l[e] : 0.0f;
        }
    };
    fetch(0);
    __syncthreads();
    float zc[NC], mm[NC], ss[NC];                                  // marginals: this lane's query at the wave's columns
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int j = wave + NW * c;
        zc[c] = (MARG && j < nz) ? zi[j * LQ + lane] : 0.0f;
        mm[c] = -__builtin_inff();
        ss[c] = 0.0f;
    }
    float mj = -__builtin_inff(), sj = 0.0f;                       // joint: this lane's query at block position `wave`

    for (int t = 0; t < n_tiles; ++t) {
        __syncthreads();                                           // the previous tile's readers are done
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int e = tid + r * kAggThreads;
            if (e < n_el) {
                const int o = dim_of[r] * LG + row_of[r];
                gm[o] = pm[r];
                gh[o] = -0.5f * expf(-pl[r]);
                gl[o] = -0.5f * pl[r];
            }
        }
        __syncthreads();
        if (t + 1 < n_tiles) fetch(t + 1);
        const long long g0 = g_lo + (long long)t * TG;
        const int ng = (int)min((long long)TG, g_hi - g0);
        const int ex_t = ex < 0 ? -1 : (int)min((long long)TG, max(-1ll, (long long)ex - g0));   // excluded row inside the tile, or outside [0, 64)

        if (MARG) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int j = wave + NW * c;
                if (j < nz) {
                    const float z = zc[c];
                    for (int b = 0; b * BL < ng; ++b) {
                        const float4* pmu = reinterpret_cast<const float4*>(gm + j * LG + b * BL);
                        const float4* phi = reinterpret_cast<const float4*>(gh + j * LG + b * BL);
                        const float4* plv = reinterpret_cast<const float4*>(gl + j * LG + b * BL);
                        const float4 m0 = pmu[0], m1 = pmu[1], h0 = phi[0], h1 = phi[1], l0 = plv[0], l1 = plv[1];
                        float l[BL] = {agg_term(z, m0.x, h0.x, l0.x), agg_term(z, m0.y, h0.y, l0.y), agg_term(z, m0.z, h0.z, l0.z),
                                       agg_term(z, m0.w, h0.w, l0.w), agg_term(z, m1.x, h1.x, l1.x), agg_term(z, m1.y, h1.y, l1.y),
                                       agg_term(z, m1.z, h1.z, l1.z), agg_term(z, m1.w, h1.w, l1.w)};
                        const int valid = ng - b * BL, off = ex_t - b * BL;
                        if (valid < BL || (unsigned)off < (unsigned)BL) agg_select(l, valid, off);
                        agg_block(l, mm[c], ss[c]);
                    }
                }
            }
        }
        if (JOINT && wave * BL < ng) {
            float acc[BL];
#pragma unroll
            for (int i = 0; i < BL; ++i) acc[i] = 0.0f;
#pragma unroll 4
            for (int j = 0; j < nz; ++j) {
                const float z = zi[j * LQ + lane];
                const float4* pmu = reinterpret_cast<const float4*>(gm + j * LG + wave * BL);
                const float4* phi = reinterpret_cast<const float4*>(gh + j * LG + wave * BL);
                const float4* plv = reinterpret_cast<const float4*>(gl + j * LG + wave * BL);
                const float4 m0 = pmu[0], m1 = pmu[1], h0 = phi[0], h1 = phi[1], l0 = plv[0], l1 = plv[1];
                acc[0] = acc[0] + agg_term(z, m0.x, h0.x, l0.x);
                acc[1] = acc[1] + agg_term(z, m0.y, h0.y, l0.y);
                acc[2] = acc[2] + agg_term(z, m0.z, h0.z, l0.z);
                acc[3] = acc[3] + agg_term(z, m0.w, h0.w, l0.w);
                acc[4] = acc[4] + agg_term(z, m1.x, h1.x, l1.x);
                acc[5] = acc[5] + agg_term(z, m1.y, h1.y, l1.y);
                acc[6] = acc[6] + agg_term(z, m1.z, h1.z, l1.z);
                acc[7] = acc[7] + agg_term(z, m1.w, h1.w, l1.w);
            }
            const int valid = ng - wave * BL, off = ex_t - wave * BL;
            if (valid < BL || (unsigned)off < (unsigned)BL) agg_select(acc, valid, off);
            agg_block(acc, mj, sj);
        }
    }

    const int cols = 1 + nz;
    float2* out = a.part + ((size_t)(q0 + lane) * a.n_slices + blockIdx.y) * cols;     // (used by lanes < nq only)
    if (MARG && lane < nq) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int j = wave + NW * c;
            if (j < nz) out[1 + j] = make_float2(mm[c], ss[c]);
        }
    }
    if (JOINT) {
        jp[wave * TQ + lane] = make_float2(mj, sj);
        __syncthreads();
        if (wave == 0 && lane < nq) {                              // the 8 block positions of a query, in position order
            float m = -__builtin_inff(), s = 0.0f;
#pragma unroll
            for (int r = 0; r < NW; ++r) {
                const float2 p = jp[r * TQ + lane];
                const float nm = __builtin_fmaxf(m, p.x);
                const float shift = nm == -__builtin_inff() ? 0.0f : nm;
                s = s * agg_exp(m - shift) + p.y * agg_exp(p.x - shift);
                m = nm;
            }
            out[0] = make_float2(m, s);
        }
    }
}

// One wave64 per query; lane c (and c + 64) combines column c of the slices' pairs in slice order in fp64, subtracts log G' and the
// constant in fp64 and rounds once.  Column 0 is the joint.  G' = 0 ("no estimate"): NaN.
__global__ void __launch_bounds__(256) k_agg_logpdf_merge(AggArgs a) {
    constexpr double kHalfLog2Pi = 0.91893853320467274178;
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.rows) return;
    const int nz = a.nz, cols = 1 + nz, ns = a.n_slices;
    int ex = a.exclude ? a.exclude[q] : -1;
    const long long counted = (long long)a.gallery_rows - ((ex >= 0 && ex < a.gallery_rows) ? 1 : 0);
    const double log_g = counted > 0 ? log((double)counted) : 0.0;
    const double inf = (double)__builtin_inff();
    for (int col = lane; col < cols; col += 64) {
        float* dst = col == 0 ? (a.joint ? a.joint + q : nullptr) : (a.marginal ? a.marginal + (size_t)q * nz + (col - 1) : nullptr);
        if (!dst) continue;
        double m = -inf, s = 0.0;
        for (int sl = 0; sl < ns; ++sl) {
            const float2 p = a.part[((size_t)q * ns + sl) * cols + col];
            const double pm = (double)p.x, nm = pm > m ? pm : m;
            const double shift = nm == -inf ? 0.0 : nm;
            s = s * exp(m - shift) + (double)p.y * exp(pm - shift);
            m = nm;
        }
        const double r = log(s) + m - log_g - (col == 0 ? (double)nz * kHalfLog2Pi : kHalfLog2Pi);
        *dst = counted > 0 ? (float)r : __builtin_nanf("");
    }
}

}  // namespace

void launch_agg_logpdf(const AggArgs& a, hipStream_t s) {
    const size_t lds = agg_lds_bytes(a.nz);
    const dim3 grid((unsigned)((a.rows + kAggQueryTile - 1) / kAggQueryTile), (unsigned)a.n_slices);
    auto go = [&](auto kernel) {
        allow_max_lds(kernel);
        launch_kernel(kernel, grid, dim3(kAggThreads), lds, s, a);
    };
    if (a.marginal && a.joint) go(k_agg_logpdf<true, true>);
    else if (a.marginal) go(k_agg_logpdf<true, false>);
    else go(k_agg_logpdf<false, true>);
}

void launch_agg_logpdf_merge(const AggArgs& a, hipStream_t s) {
    launch_kernel(k_agg_logpdf_merge, dim3((unsigned)((a.rows + 3) / 4)), dim3(256), 0, s, a);
}

}  // namespace avae
