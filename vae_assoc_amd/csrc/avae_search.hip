// Black-box search kernels (avae_search.h, include/avae.h): k_search_sample, k_search_update.
#include "avae_device.h"
#include "avae_philox.h"
#include "avae_search.h"

namespace avae {

namespace {

// Every operation below is the one written (a fused multiply-add only where __builtin_fmaf says so): tests/search_reference.py
// restates them one by one.
#pragma clang fp contract(off)

__global__ __launch_bounds__(kSearchThreads) void k_search_sample(const SearchSampleArgs a) {
    __shared__ float y[kSearchTileFloats];
    const int tid = threadIdx.x, n = a.n, nq = search_quads(n), TR = search_tile_rows(n);
    const long long r0 = (long long)blockIdx.x * TR;
    const int nrows = (int)(a.rows - r0 < TR ? a.rows - r0 : TR);

    for (int item = tid; item < nrows * nq; item += kSearchThreads) {
        const int lr = item / nq, q = item - lr * nq;
        const long long row = r0 + lr;
        const long long p = row / a.R;
        const unsigned r = (unsigned)(row - p * a.R);
        unsigned w[4];
        float nrm[4];
        philox4x32_10(a.problem0 + (unsigned)p, r, (unsigned)q, a.iteration, (unsigned)a.seed, (unsigned)(a.seed >> 32) ^ kSearchSalt, w);
        box_muller4(w, nrm);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int d = 4 * q + e;
            if (d < n) y[lr * n + d] = __builtin_fmaf(sqrtf(a.var[(size_t)p * n + d]), nrm[e], a.mean[(size_t)p * n + d]);
        }
    }
    __syncthreads();
    float* out = a.x + (size_t)r0 * n;
    if (!a.proj_A) {
        for (int i = tid; i < nrows * n; i += kSearchThreads) out[i] = y[i];
        return;
    }
    const int g = a.g;
    for (int i = tid; i < nrows * n; i += kSearchThreads) {
        const int lr = i / n, d = i - lr * n, grp = d / g, j = d - grp * g;
        const long long p = (r0 + lr) / a.R;
        const float* A = a.proj_A + ((size_t)grp * g + j) * g;
        const float* yy = y + lr * n + grp * g;
        float acc = a.proj_b[(size_t)p * n + d];
        for (int k = 0; k < g; ++k) acc = __builtin_fmaf(A[k], yy[k], acc);
        out[i] = acc;
    }
}

// THE TREE of avae_search.h over the workgroup's 256 values; every thread gets the result
template <typename T, typename F>
__device__ __forceinline__ T tree(T* red, T v, F&& op) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = kSearchThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = op(red[tid], red[tid + s]);
        __syncthreads();
    }
    const T out = red[0];
    __syncthreads();
    return out;
}

struct Stat { float mn, mx; int bi, cnt; };      // minimum and maximum of the counting costs, the best rollout, their number

__global__ __launch_bounds__(kSearchThreads) void k_search_update(const SearchUpdateArgs a) {
    __shared__ double w_s[kSearchMaxR];
    __shared__ float c_s[kSearchMaxR];             // the counting costs; NaN where a rollout does not count
    __shared__ double red_d[kSearchThreads];
    __shared__ Stat red_s[kSearchThreads];
    const int tid = threadIdx.x, R = a.R, n = a.n;
    const size_t p = blockIdx.x;
    const float* x = a.x + p * (size_t)R * n;
    const float best_old = a.best_cost[p];
    const bool frozen = a.frozen[p] != 0;
    const double inf = __builtin_inf();
    auto add = [](double u, double v) { return u + v; };

    // 1. the counting rollouts
    Stat st = {__builtin_inff(), -__builtin_inff(), 0x7fffffff, 0};
    for (int r = tid; r < R; r += kSearchThreads) {
        const float c = a.cost[p * R + r];
        const bool ok = __builtin_isfinite(c);
        c_s[r] = ok ? c : __builtin_nanf("");
        if (ok) {
            if (c < st.mn) { st.mn = c; st.bi = r; }
            if (c > st.mx) st.mx = c;
            ++st.cnt;
        }
    }
    st = tree(red_s, st, [](const Stat& u, const Stat& v) {
        Stat o;
        const bool take = v.mn < u.mn || (v.mn == u.mn && v.bi < u.bi);
        o.mn = take ? v.mn : u.mn; o.bi = take ? v.bi : u.bi;
        o.mx = v.mx > u.mx ? v.mx : u.mx;
        o.cnt = u.cnt + v.cnt;
        return o;
    });
    const int F = st.cnt;
    if (F > 0 && st.mn < best_old) {
        for (int d = tid; d < n; d += kSearchThreads) a.best_x[p * n + d] = x[(size_t)st.bi * n + d];
        if (tid == 0) a.best_cost[p] = st.mn;
    }
    // 2.
    if (F == 0 || frozen) {
        if (tid == 0) {
            if (a.avg_cost) a.avg_cost[p] = __builtin_nanf("");
            if (a.min_cost) a.min_cost[p] = __builtin_nanf("");
            if (a.moved) a.moved[p] = __builtin_nanf("");
        }
        return;
    }
    const double cmin = (double)st.mn, cmax = (double)st.mx;

    // 3. mean and standard deviation of the counting costs
    double t = 0.0;
    for (int r = tid; r < R; r += kSearchThreads) {
        const float c = c_s[r];
        if (c == c) t = t + (double)c;
    }
    const double cbar = tree(red_d, t, add) / (double)F;
    t = 0.0;
    for (int r = tid; r < R; r += kSearchThreads) {
        const float c = c_s[r];
        if (c == c) { const double e = (double)c - cbar; t = t + e * e; }
    }
    const double sd = sqrt(tree(red_d, t, add) / (double)F);

    // 4. weights
    const bool equal = sd <= 1e-8 * fabs(cbar);
    t = 0.0;
    for (int r = tid; r < R; r += kSearchThreads) {
        const float c = c_s[r];
        double w = 0.0;
        if (c == c) {
            if (equal) {
                w = 1.0;
            } else if (a.weighting == AVAE_SEARCH_PIBB) {
                w = exp(-a.h * ((double)c - cmin) / ((cmax - cmin) + 1e-6));
            } else {
                int rank = 0;
                for (int j = 0; j < R; ++j) {
                    const float cj = c_s[j];
                    rank += (cj < c || (cj == c && j < r)) ? 1 : 0;
                }
                if (rank < a.mu) w = a.weighting == AVAE_SEARCH_CEM ? 1.0 / (double)a.mu : log((double)a.mu + 0.5) - log((double)(rank + 1));
            }
            t = t + w;
        }
        w_s[r] = w;
    }
    const double W = tree(red_d, t, add);
    for (int r = tid; r < R; r += kSearchThreads) w_s[r] = w_s[r] / W;
    __syncthreads();

    // 5. the weighted mean and variance of a thread's dimensions
    double m0[kSearchDims], v0[kSearchDims], m1[kSearchDims], s[kSearchDims];
#pragma unroll
    for (int k = 0; k < kSearchDims; ++k) {
        const int d = tid + k * kSearchThreads;
        m0[k] = d < n ? (double)a.mean[p * n + d] : 0.0;
        v0[k] = d < n ? (double)a.var[p * n + d] : 0.0;
        m1[k] = 0.0; s[k] = 0.0;
    }
    for (int r = 0; r < R; ++r) {
        const double w = w_s[r];
        if (w == 0.0) continue;
#pragma unroll
        for (int k = 0; k < kSearchDims; ++k) {
            const int d = tid + k * kSearchThreads;
            if (d < n) m1[k] = m1[k] + w * (double)x[(size_t)r * n + d];
        }
    }
    const bool cem_cov = a.cov_update == AVAE_SEARCH_CEM;
    for (int r = 0; r < R; ++r) {
        const double w = w_s[r];
        if (w == 0.0) continue;
#pragma unroll
        for (int k = 0; k < kSearchDims; ++k) {
            const int d = tid + k * kSearchThreads;
            if (d < n) {
                const double e = (double)x[(size_t)r * n + d] - (cem_cov ? m1[k] : m0[k]);
                s[k] = s[k] + w * (e * e);
            }
        }
    }
    // 6. bounds
    double v1[kSearchDims], vmax = -inf, mv = 0.0;
#pragma unroll
    for (int k = 0; k < kSearchDims; ++k) {
        const int d = tid + k * kSearchThreads;
        v1[k] = (1.0 - a.lr) * v0[k] + a.lr * s[k];
        if (a.abs_upper >= 0.0 && v1[k] > a.abs_upper) v1[k] = a.abs_upper;
        if (d < n) {
            if (v1[k] > vmax) vmax = v1[k];
            const double e = m1[k] - m0[k];
            mv = mv + e * e;
        }
    }
    if (a.rel_lower >= 0.0 || a.abs_lower >= 0.0) {
        double lower = a.abs_lower;
        if (a.rel_lower >= 0.0) {
            vmax = tree(red_d, vmax, [](double u, double v) { return v > u ? v : u; });
            const double rel = a.rel_lower * vmax;
            lower = (a.abs_lower >= 0.0 && !(rel > a.abs_lower)) ? a.abs_lower : rel;
        }
#pragma unroll
        for (int k = 0; k < kSearchDims; ++k)
            if (v1[k] < lower) v1[k] = lower;
    }
    // 7. 8.
    const double moved = sqrt(tree(red_d, mv, add));
#pragma unroll
    for (int k = 0; k < kSearchDims; ++k) {
        const int d = tid + k * kSearchThreads;
        if (d < n) {
            a.mean[p * n + d] = (float)m1[k];
            a.var[p * n + d] = (float)v1[k];
        }
    }
    if (tid == 0) {
        a.n_applied[p] = a.n_applied[p] + 1;
        if (a.avg_cost) a.avg_cost[p] = (float)cbar;
        if (a.min_cost) a.min_cost[p] = (float)cmin;
        if (a.moved) a.moved[p] = (float)moved;
        if (moved < a.tol) a.frozen[p] = 1;
    }
}

}  // namespace

void launch_search_sample(const SearchSampleArgs& a, hipStream_t s) {
    const int TR = search_tile_rows(a.n);
    const long long tiles = (a.rows + TR - 1) / TR;
    launch_kernel(k_search_sample, dim3((unsigned)tiles), dim3(kSearchThreads), 0, s, a);
}

void launch_search_update(const SearchUpdateArgs& a, int P, hipStream_t s) {
    launch_kernel(k_search_update, dim3((unsigned)P), dim3(kSearchThreads), 0, s, a);
}

}  // namespace avae
