// Per-dimension posterior diagnostics of libavae (gfx950): avae_latent_stats in include/avae.h; the plan, the scratch layout and
// the launch shapes: avae_latent_stats.h; DESIGN.md section 19.
#include "avae_device.h"
#include "avae_latent_stats.h"

namespace avae {

namespace {

// Every operation below is the one written (a fused multiply-add only where __builtin_fma says so): the bits of an entry must not
// depend on how many modalities the call carries.
#pragma clang fp contract(off)

// How the 256 threads of a workgroup share a slice's elements: column j = tid % nzp (idle for j >= nz), row group g = tid / nzp of
// G = 256 / nzp, nzp the power of two >= nz (at least 8).  Thread (g, j) takes rows g, g + G, ... of its column in row order.
struct Lanes { int nzp, G, j, g; };
__device__ __forceinline__ Lanes lanes_of(int nz) {
    Lanes l;
    l.nzp = nz <= 8 ? 8 : nz <= 16 ? 16 : nz <= 32 ? 32 : 64;
    l.G = kStatsThreads / l.nzp;
    l.j = threadIdx.x & (l.nzp - 1);
    l.g = threadIdx.x / l.nzp;
    return l;
}

// First row of [lo, hi) that has modality m1 (and m2, if >= 0), or -1.  The minimum of the threads' own first hits: no order to fix.
__device__ long long first_row(const StatsArgs& a, long long lo, long long hi, int m1, int m2, long long* s_first) {
    const int tid = threadIdx.x;
    long long f = hi;
    if (!a.present) {
        f = lo;
    } else {
        for (long long row = lo + tid; row < hi; row += kStatsThreads) {
            const uint8_t* p = a.present + row * a.n_mod;
            if (p[m1] != 0 && (m2 < 0 || p[m2] != 0)) { f = row; break; }
        }
    }
    s_first[tid] = f;
    __syncthreads();
    for (int o = kStatsThreads / 2; o > 0; o >>= 1) {
        if (tid < o) { const long long x = s_first[tid + o]; if (x < s_first[tid]) s_first[tid] = x; }
        __syncthreads();
    }
    f = s_first[0];
    __syncthreads();
    return f < hi ? f : -1;
}

// sums[q] of every thread -> red; then thread (0, j) adds its column's G values in group order and returns them in sums[q].
template <int NQ>
__device__ __forceinline__ void column_totals(const Lanes& l, double (&sums)[NQ], double* red) {
    static_assert(NQ <= kStatsMaxSums, "red holds kStatsMaxSums values per thread");
#pragma unroll
    for (int q = 0; q < NQ; ++q) red[q * kStatsThreads + threadIdx.x] = sums[q];
    __syncthreads();
    if (l.g == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            double t = 0.0;
            for (int gg = 0; gg < l.G; ++gg) t += red[q * kStatsThreads + gg * l.nzp + l.j];
            sums[q] = t;
        }
    }
}

// The item of modality m: column sums over the rows that have m, and the Gram of the shifted means.
__device__ void stats_modality(const StatsArgs& a, int slice, int m, float* tile, double* red, long long* s_first) {
    const int nz = a.nz, tid = threadIdx.x;
    const Lanes l = lanes_of(nz);
    const float* mu = a.mu[m];
    const float* lv = a.lv[m];
    if (!mu) return;                                               // absent everywhere: the merge never looks at this partial
    double* part = a.scratch + ((size_t)slice * a.n_mod + m) * stats_mod_stride(nz);
    const long long lo = (long long)slice * a.row_tile, hi = min(a.rows, lo + a.row_tile);
    const long long first = first_row(a, lo, hi, m, -1, s_first);
    if (first < 0) { if (tid == 0) part[0] = 0.0; return; }
    const bool col = l.j < nz;
    const double c = col ? (double)mu[first * nz + l.j] : 0.0;
    double sums[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                    // d, d*d, exp(lv), kl, rows
    // the Gram: thread (ti, tj) of 16 x 16 holds the 4 x 4 block at (4 ti, 4 tj)
    const int ti = tid >> 4, tj = tid & 15;
    const bool gram = a.want_cov && 4 * ti < nz && 4 * tj < nz;
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int w = 0; w < 4; ++w) acc[u][w] = 0.0;

    for (long long r0 = lo; r0 < hi; r0 += kStatsChunk) {
        const int nr = (int)min((long long)kStatsChunk, hi - r0);
        if (a.want_cov) __syncthreads();                           // the previous tile's readers are done
        for (int r = l.g; r < nr; r += l.G) {
            const long long row = r0 + r;
            const bool has = !a.present || a.present[row * a.n_mod + m] != 0;
            float dev = 0.0f;                                       // an absent row is a row of zeros in the tile: selected, never read
            if (has) sums[4] += 1.0;
            if (has && col) {
                const float x = mu[row * nz + l.j], lg = lv[row * nz + l.j];
                const double d = (double)x - c, v = (double)expf(lg);
                sums[0] += d;
                sums[1] = __builtin_fma(d, d, sums[1]);
                sums[2] += v;
                sums[3] += 0.5 * ((double)x * (double)x + v - (double)lg - 1.0);
                dev = (float)d;
            }
            if (a.want_cov) tile[r * kStatsLd + l.j] = dev;        // columns nz .. nzp - 1: zeros
        }
        if (a.want_cov) __syncthreads();
        if (gram) {
            for (int r = 0; r < nr; ++r) {
                const float4 p = *reinterpret_cast<const float4*>(tile + r * kStatsLd + 4 * ti);
                const float4 q = *reinterpret_cast<const float4*>(tile + r * kStatsLd + 4 * tj);
                const double pa[4] = {(double)p.x, (double)p.y, (double)p.z, (double)p.w};
                const double qa[4] = {(double)q.x, (double)q.y, (double)q.z, (double)q.w};
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int w = 0; w < 4; ++w) acc[u][w] = __builtin_fma(pa[u], qa[w], acc[u][w]);
            }
        }
    }
    column_totals(l, sums, red);
    if (l.g == 0 && col) {
        if (l.j == 0) part[0] = sums[4];
        part[1 + l.j] = c;
#pragma unroll
        for (int q = 0; q < 4; ++q) part[1 + (1 + q) * nz + l.j] = sums[q];
    }
    if (gram) {
        double* G = part + 1 + 5 * nz;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int w = 0; w < 4; ++w)
                if (4 * ti + u < nz && 4 * tj + w < nz) G[(4 * ti + u) * nz + 4 * tj + w] = acc[u][w];
    }
}

// The item of the pair s < d: column sums of both sides over the rows that have both.
__device__ void stats_pair(const StatsArgs& a, int slice, int s, int d, double* red, long long* s_first) {
    const int nz = a.nz, tid = threadIdx.x;
    const Lanes l = lanes_of(nz);
    const float *ms = a.mu[s], *ls = a.lv[s], *md = a.mu[d], *ld = a.lv[d];
    if (!ms || !md) return;
    double* part = a.scratch + (size_t)a.n_slices * a.n_mod * stats_mod_stride(nz) +
                   ((size_t)slice * stats_pairs(a.n_mod) + stats_pair_index(a.n_mod, s, d)) * stats_pair_stride(nz);
    const long long lo = (long long)slice * a.row_tile, hi = min(a.rows, lo + a.row_tile);
    const long long first = first_row(a, lo, hi, s, d, s_first);
    if (first < 0) { if (tid == 0) part[0] = 0.0; return; }
    const bool col = l.j < nz;
    const double cs = col ? (double)ms[first * nz + l.j] : 0.0, cd = col ? (double)md[first * nz + l.j] : 0.0;
    double sums[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};           // d_s, d_d, d_s*d_s, d_d*d_d, d_s*d_d, assoc, rows
    for (long long row = lo + l.g; row < hi; row += l.G) {
        const bool has = !a.present || (a.present[row * a.n_mod + s] != 0 && a.present[row * a.n_mod + d] != 0);
        if (!has) continue;
        sums[6] += 1.0;
        if (!col) continue;
        const long long e = row * nz + l.j;
        const float xs = ms[e], xd = md[e], gs = ls[e], gd = ld[e];
        const double vs = (double)expf(gs), is = (double)expf(-gs), vd = (double)expf(gd), id = (double)expf(-gd);
        const double ds = (double)xs - cs, dd = (double)xd - cd;
        const double t = vs - vd, df = (double)xs - (double)xd;
        sums[0] += ds;
        sums[1] += dd;
        sums[2] = __builtin_fma(ds, ds, sums[2]);
        sums[3] = __builtin_fma(dd, dd, sums[3]);
        sums[4] = __builtin_fma(ds, dd, sums[4]);
        sums[5] += 0.5 * ((t * is) * (t * id) + (df * df) * (is + id));
    }
    column_totals(l, sums, red);
    if (l.g == 0 && col) {
        if (l.j == 0) part[0] = sums[6];
        part[1 + l.j] = cs;
        part[1 + nz + l.j] = cd;
#pragma unroll
        for (int q = 0; q < 6; ++q) part[1 + (2 + q) * nz + l.j] = sums[q];
    }
}

// grid (row slices, n_mod modality items + the pair items)
__global__ void __launch_bounds__(kStatsThreads) k_latent_stats(StatsArgs a) {
    __shared__ __attribute__((aligned(16))) float tile[kStatsChunk * kStatsLd];
    __shared__ double red[kStatsMaxSums * kStatsThreads];
    __shared__ long long s_first[kStatsThreads];
    const int slice = blockIdx.x, item = blockIdx.y;
    if (item < a.n_mod) { stats_modality(a, slice, item, tile, red, s_first); return; }
    int p = item - a.n_mod, s = 0;
    while (p >= a.n_mod - 1 - s) { p -= a.n_mod - 1 - s; ++s; }
    stats_pair(a, slice, s, s + 1 + p, red, s_first);
}

// Running (count, mean of a, mean of b, M2 of a, co-moment of a and b), and one slice's added to it: Chan's pairwise update.
struct Moments { double n = 0.0, ma = 0.0, mb = 0.0, m2 = 0.0, c = 0.0; };
__device__ __forceinline__ void chan_add(Moments& r, double n, double ca, double sa, double qa, double cb, double sb, double pab) {
    const double ma = ca + sa / n, mb = cb + sb / n;               // a slice's sums are of values shifted by (ca, cb)
    const double m2 = qa - sa * sa / n, c = pab - sa * sb / n;
    if (r.n == 0.0) { r.n = n; r.ma = ma; r.mb = mb; r.m2 = m2; r.c = c; return; }
    const double N = r.n + n, da = ma - r.ma, db = mb - r.mb, w = r.n * n / N;
    r.ma += da * (n / N);
    r.mb += db * (n / N);
    r.m2 += m2 + da * da * w;
    r.c += c + da * db * w;
    r.n = N;
}

// One thread per entry of the [M][M][nz] tables (the diagonal ones also write post_var and kl, column 0 the count), then one per
// entry of cov.
__global__ void __launch_bounds__(256) k_latent_stats_merge(StatsArgs a) {
    const int M = a.n_mod, nz = a.nz;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n_table = (long long)M * M * nz;
    const double nan = __builtin_nan("");
    const size_t ms = stats_mod_stride(nz), ps = stats_pair_stride(nz);
    const double* pair_base = a.scratch + (size_t)a.n_slices * M * ms;
    const int P = stats_pairs(M);
    if (t < n_table) {
        const int s = (int)(t / ((long long)M * nz)), d = (int)(t / nz) % M, j = (int)(t % nz);
        Moments r;
        double sum_v = 0.0, sum_kl = 0.0, sum_assoc = 0.0;
        if (s == d) {
            if (a.mu[s])
                for (int k = 0; k < a.n_slices; ++k) {
                    const double* p = a.scratch + ((size_t)k * M + s) * ms;
                    const double n = p[0];
                    if (n == 0.0) continue;
                    chan_add(r, n, p[1 + j], p[1 + nz + j], p[1 + 2 * nz + j], p[1 + j], p[1 + nz + j], p[1 + 2 * nz + j]);
                    sum_v += p[1 + 3 * nz + j];
                    sum_kl += p[1 + 4 * nz + j];
                }
        } else if (a.mu[s] && a.mu[d]) {
            const int lo = s < d ? s : d, hi = s < d ? d : s;
            const int A = s < d ? 0 : 1, B = 1 - A;                // which side of the partial mu_s is
            const int pi = stats_pair_index(M, lo, hi);
            for (int k = 0; k < a.n_slices; ++k) {
                const double* p = pair_base + ((size_t)k * P + pi) * ps;
                const double n = p[0];
                if (n == 0.0) continue;
                chan_add(r, n, p[1 + A * nz + j], p[1 + (2 + A) * nz + j], p[1 + (4 + A) * nz + j],
                         p[1 + B * nz + j], p[1 + (2 + B) * nz + j], p[1 + 6 * nz + j]);
                sum_assoc += p[1 + 7 * nz + j];
            }
        }
        const bool any = r.n > 0.0;
        double var = r.m2 / r.n;
        if (var < 0.0) var = 0.0;                                  // (a NaN stays a NaN)
        const size_t o = ((size_t)s * M + d) * nz + j;
        if (a.out.mean) a.out.mean[o] = any ? r.ma : nan;
        if (a.out.var) a.out.var[o] = any ? var : nan;
        if (a.out.xcov) a.out.xcov[o] = any ? (s == d ? var : r.c / r.n) : nan;
        if (a.out.assoc) a.out.assoc[o] = any ? (s == d ? 0.0 : sum_assoc / r.n) : nan;
        if (j == 0 && a.out.count) a.out.count[(size_t)s * M + d] = (long long)r.n;
        if (s == d) {
            if (a.out.post_var) a.out.post_var[(size_t)s * nz + j] = any ? sum_v / r.n : nan;
            if (a.out.kl) a.out.kl[(size_t)s * nz + j] = any ? sum_kl / r.n : nan;
        }
        return;
    }
    const long long e = t - n_table;
    if (!a.want_cov || e >= (long long)M * nz * nz) return;
    const int m = (int)(e / ((long long)nz * nz)), i = (int)(e / nz) % nz, j = (int)(e % nz);
    Moments r;
    if (a.mu[m])
        for (int k = 0; k < a.n_slices; ++k) {
            const double* p = a.scratch + ((size_t)k * M + m) * ms;
            const double n = p[0];
            if (n == 0.0) continue;
            chan_add(r, n, p[1 + i], p[1 + nz + i], p[1 + 2 * nz + i], p[1 + j], p[1 + nz + j], p[1 + 5 * nz + (size_t)i * nz + j]);
        }
    double c = r.c / r.n;
    if (i == j && c < 0.0) c = 0.0;
    a.out.cov[e] = r.n > 0.0 ? c : nan;
}

}  // namespace

void launch_latent_stats(const StatsArgs& a, hipStream_t s) {
    launch_kernel(k_latent_stats, dim3((unsigned)a.n_slices, (unsigned)(a.n_mod + stats_pairs(a.n_mod))), dim3(kStatsThreads), 0, s, a);
}

void launch_latent_stats_merge(const StatsArgs& a, hipStream_t s) {
    const long long entries = (long long)a.n_mod * a.n_mod * a.nz + (a.want_cov ? (long long)a.n_mod * a.nz * a.nz : 0);
    launch_kernel(k_latent_stats_merge, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace avae
