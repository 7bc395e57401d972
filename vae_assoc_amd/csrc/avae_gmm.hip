// Mixture-prior kernels of libavae (gfx950): EM for a diagonal Gaussian mixture fitted to Gaussian-uncertain inputs, and the
// per-row score under it (avae_gmm_fit / avae_gmm_score in include/avae.h; the plan, the scratch and the launch shapes:
// avae_gmm.h).  The rows x K x n_z tensor of exponents lives in registers only.
#include "avae_device.h"
#include "avae_gmm.h"

namespace avae {

namespace {

// Every float operation below is the one written (a fused multiply-add only where __builtin_fmaf says so): the bits of a row's
// outputs must not depend on which lane, wave or tile formed them.
#pragma clang fp contract(off)

constexpr float kLog2PiF = 1.83787706640934548356f;

// grid = row slices, kGmmThreads threads.  STATS 0: per-row outputs only (avae_gmm_score); 1: the slice's sufficient statistics;
// 2: the slice's sum of ll and used-row count only (the pass that scores the returned parameters).
template <int STATS>
__global__ void __launch_bounds__(kGmmThreads) k_gmm_estep(GmmArgs a) {
    constexpr int T = kGmmTile, LD = kGmmTileLd, NW = kGmmWaves, OWN = kGmmOwn, CH = 4, NCH = OWN / CH;
    constexpr int PER = T * kGmmMaxNz / kGmmThreads;              // staged elements per thread and tile, at most (16)
    static_assert(T == 64 && NCH * CH * NW == kGmmMaxK, "lane = row; a wave takes the components in chunks of CH");
    extern __shared__ __attribute__((aligned(16))) unsigned char gmm_lds[];
    const int nz = a.nz, K = a.K, K1 = K + 1;
    float2* pm = reinterpret_cast<float2*>(gmm_lds);               // [K][nz] (m, -0.5 * expf(-s))
    float* mt = reinterpret_cast<float*>(pm + K * nz);             // [nz][LD] mu
    float* vt = mt + nz * LD;                                      // [nz][LD] expf(lv), or 0
    float* rt = vt + nz * LD;                                      // [T][K + 1] exponents, then p, then r
    float* ck = rt + T * K1;                                       // [K] log pi_k - 0.5 * sum_j (s_kj + log 2pi)
    int* s_bad = reinterpret_cast<int*>(ck + K);                   // [T] 1: the row holds a non-finite entry
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long lo = (long long)blockIdx.x * a.slice_rows, hi = min(a.rows, lo + a.slice_rows);
    const int n_tiles = (int)((hi - lo + T - 1) / T);             // >= 1: no slice is empty
    const int n_el = T * nz;
    const float nanv = __builtin_nanf("");

    float fm[PER], fl[PER];                                        // the next tile on its way from memory
    auto fetch = [&](int t) {
        const long long r0 = lo + (long long)t * T;
        const int cnt = (int)min((long long)T, hi - r0) * nz;
        const float* m = a.mu + (size_t)r0 * nz;
        const float* l = a.lv ? a.lv + (size_t)r0 * nz : nullptr;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = tid + i * kGmmThreads;
            const bool in = e < cnt;
            fm[i] = in ? m[e] : 0.0f;                              // rows past the end: zeros (finite arithmetic, r = 0)
            fl[i] = (in && l) ? l[e] : 0.0f;
        }
    };
    fetch(0);

    for (int e = tid; e < K * nz; e += kGmmThreads) pm[e] = make_float2(a.m_in[e], -0.5f * expf(-a.s_in[e]));
    if (tid < K) {
        float acc = 0.0f;
        for (int j = 0; j < nz; ++j) acc = acc + (a.s_in[tid * nz + j] + kLog2PiF);
        ck[tid] = logf(a.w_in[tid]) - 0.5f * acc;
    }

    // phase 2's share of a thread: column pj (idle for pj >= nz) and the components pg, pg + KG, ...
    const int JW = nz <= 8 ? 8 : nz <= 16 ? 16 : nz <= 32 ? 32 : 64, KG = kGmmThreads / JW;
    const int pj = tid & (JW - 1), pg = tid / JW;
    const int pjj = pj < nz ? pj : nz - 1;                         // (an idle thread reads a valid column and writes nothing)
    double S1[OWN], S2[OWN], RR[OWN], sum_ll = 0.0;                // sum_ll, used: wave 0, lane = row of every tile
    double mk[OWN];
    int kk[OWN], used = 0;
    if (STATS == 1) {
#pragma unroll
        for (int c = 0; c < OWN; ++c) {
            S1[c] = 0.0; S2[c] = 0.0; RR[c] = 0.0;
            kk[c] = min(pg + KG * c, K - 1);
            mk[c] = (double)a.m_in[kk[c] * nz + pjj];
        }
    }

    for (int t = 0; t < n_tiles; ++t) {
        const long long r0 = lo + (long long)t * T;
        const int nr = (int)min((long long)T, hi - r0);
        __syncthreads();                                           // the previous tile's readers are done (and pm, ck are written)
        if (tid < T) s_bad[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = tid + i * kGmmThreads;
            if (e < n_el) {
                const int row = e / nz, j = e - row * nz;
                const float x = fm[i], g = fl[i];
                if (!latent_finite(x) || !latent_finite(g)) s_bad[row] = 1;
                mt[j * LD + row] = x;
                vt[j * LD + row] = a.lv ? expf(g) : 0.0f;          // (rows past the end: expf(0) = 1, finite; r = 0)
            }
        }
        __syncthreads();
        if (t + 1 < n_tiles) fetch(t + 1);
        // a row with a non-finite entry is selected away: its staged values become zeros and its r becomes 0, so that it adds
        // +-0 to every sum -- no bit of a sum depends on what it held
        const unsigned long long badm = __ballot(s_bad[lane] != 0);
        if (badm != 0ull) {
            for (int e = tid; e < n_el; e += kGmmThreads) {
                const int row = e / nz, j = e - row * nz;
                if ((badm >> row) & 1ull) { mt[j * LD + row] = 0.0f; vt[j * LD + row] = 0.0f; }
            }
            __syncthreads();
        }
        const bool bad = ((badm >> lane) & 1ull) != 0, unused = bad || lane >= nr;

        // ---- phase 1: lane = row; wave w takes the components [4w, 4w + 4), [4w + 16, 4w + 20), ...
        float pv[NCH][CH];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const int k0 = wave * CH + ch * NW * CH;
            if (k0 < K) {
                const float2* q[CH];
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int k = min(k0 + i, K - 1);              // (a chunk past K repeats the last component, unwritten)
                    q[i] = pm + k * nz;
                    pv[ch][i] = ck[k];
                }
#pragma unroll 4
                for (int j = 0; j < nz; ++j) {
                    const float x = mt[j * LD + lane], v = vt[j * LD + lane];
#pragma unroll
                    for (int i = 0; i < CH; ++i) {
                        const float2 p = q[i][j];
                        const float d = x - p.x;
                        pv[ch][i] = __builtin_fmaf(__builtin_fmaf(d, d, v), p.y, pv[ch][i]);
                    }
                }
#pragma unroll
                for (int i = 0; i < CH; ++i)
                    if (k0 + i < K) rt[lane * K1 + k0 + i] = pv[ch][i];
            }
        }
        __syncthreads();
        float mx = -__builtin_inff();
#pragma unroll 8
        for (int k = 0; k < K; ++k) mx = __builtin_fmaxf(mx, rt[lane * K1 + k]);
        const float shift = mx == -__builtin_inff() ? 0.0f : mx;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
            if (wave * CH + ch * NW * CH < K) {
#pragma unroll
                for (int i = 0; i < CH; ++i) pv[ch][i] = expf(pv[ch][i] - shift);
            }
        __syncthreads();
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const int k0 = wave * CH + ch * NW * CH;
#pragma unroll
            for (int i = 0; i < CH; ++i)
                if (k0 + i < K) rt[lane * K1 + k0 + i] = pv[ch][i];
        }
        __syncthreads();
        // the K terms in k order in fp64, rounded once: with r = p / sum correctly rounded, a row of r sums to 1 within 2^-23
        // whatever K is (an fp32 running sum of 64 terms is off by several ulp, and every r of the row with it)
        double sum64 = 0.0;
#pragma unroll 8
        for (int k = 0; k < K; ++k) sum64 += (double)rt[lane * K1 + k];
        const float sum = (float)sum64;
        __syncthreads();
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const int k0 = wave * CH + ch * NW * CH;
#pragma unroll
            for (int i = 0; i < CH; ++i)
                if (k0 + i < K) rt[lane * K1 + k0 + i] = unused ? 0.0f : pv[ch][i] / sum;
        }
        const float ll = shift + logf(sum);
        if (STATS != 0 && wave == 0 && !unused) { sum_ll += (double)ll; ++used; }
        __syncthreads();

        // ---- per-row outputs
        if (STATS == 0) {
            if (a.ll && wave == 0 && lane < nr) a.ll[r0 + lane] = bad ? nanv : ll;
            if (a.component && wave == 1 && lane < nr) {
                int best = -1;
                if (!bad) {
                    float bv = rt[lane * K1];
                    best = 0;
                    for (int k = 1; k < K; ++k) {
                        const float r = rt[lane * K1 + k];
                        if (r > bv) { bv = r; best = k; }
                    }
                }
                a.component[r0 + lane] = best;
            }
            if (a.resp) {
                float* dst = a.resp + (size_t)r0 * K;
                for (int e = tid; e < nr * K; e += kGmmThreads) {
                    const int row = e / K, k = e - row * K;
                    dst[e] = ((badm >> row) & 1ull) ? nanv : rt[row * K1 + k];
                }
            }
        }

        // ---- phase 2: thread = column pj and the components pg, pg + KG, ...; the tile's rows in order
        // In fp64: d = mu - m and the products r d, d d are then exact, so the M-step's S2 / R - (S1 / R)^2 cancels d^2 against
        // itself and not against its fp32 rounding (one row with d^2 >> v: the variance is v, not v +- 1e-7 d^2).  An fp64
        // fused multiply-add issues at the rate of an unpacked fp32 one.
        if (STATS == 1) {
#pragma unroll 2
            for (int row = 0; row < nr; ++row) {
                const double x = (double)mt[pjj * LD + row], v = (double)vt[pjj * LD + row];
                const float* rr = rt + row * K1;
#pragma unroll
                for (int c = 0; c < OWN; ++c) {
                    if (c * KG < K) {
                        const double r = (double)rr[kk[c]];
                        const double d = x - mk[c];
                        S1[c] = __builtin_fma(r, d, S1[c]);
                        S2[c] = __builtin_fma(r, __builtin_fma(d, d, v), S2[c]);
                        RR[c] = RR[c] + r;
                    }
                }
            }
        }
    }

    if (STATS != 0) {
        double* part = a.part + (size_t)blockIdx.x * gmm_part_stride(K, nz);
        // the 64 row positions' sums of ll and row counts, in position order
        __syncthreads();
        double* red = reinterpret_cast<double*>(rt);               // (64 doubles fit the r tile of any K >= 1; 8-byte aligned)
        if (wave == 0) { red[lane] = sum_ll; s_bad[lane] = used; }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            long long n = 0;
            for (int i = 0; i < T; ++i) { s += red[i]; n += s_bad[i]; }
            part[0] = s; part[1] = (double)n;
        }
        if (STATS == 1) {
#pragma unroll
            for (int c = 0; c < OWN; ++c) {
                const int k = pg + KG * c;
                if (k < K && pj < nz) {
                    if (pj == 0) part[2 + k] = RR[c];
                    part[2 + K + (size_t)k * nz + pj] = S1[c];
                    part[2 + K + (size_t)K * nz + (size_t)k * nz + pj] = S2[c];
                }
            }
        }
    }
}

// grid = blocks of 256 of the K * n_z entries (one block for the last merge): the slices' partials in slice order in fp64, then
// the update of one (k, j) per thread.  Every block sums R, ll and the row count for itself; block 0 writes the weights and the bound.
__global__ void __launch_bounds__(kGmmThreads) k_gmm_mstep(GmmArgs a) {
    __shared__ double s_R[kGmmMaxK];
    __shared__ double s_tot[3];                                    // sum_k R_k | sum ll | used rows
    const int tid = threadIdx.x, nz = a.nz, K = a.K, ns = a.n_slices;
    const size_t stride = gmm_part_stride(K, nz);
    if (!a.final_pass && tid < K) {
        double R = 0.0;
        const double* p = a.part + 2 + tid;
#pragma unroll 8
        for (int sl = 0; sl < ns; ++sl) R += p[sl * stride];
        s_R[tid] = R;
    }
    if (tid == 64) {
        double sll = 0.0, cnt = 0.0;
#pragma unroll 8
        for (int sl = 0; sl < ns; ++sl) { sll += a.part[sl * stride]; cnt += a.part[sl * stride + 1]; }
        s_tot[1] = sll; s_tot[2] = cnt;
    }
    __syncthreads();
    if (tid == 0 && !a.final_pass) {
        double t = 0.0;
        for (int k = 0; k < K; ++k) t += s_R[k];
        s_tot[0] = t;
    }
    __syncthreads();
    const double cnt = s_tot[2];
    const bool any = cnt > 0.0;
    if (tid == 0 && blockIdx.x == 0) {
        a.bound[0] = any ? s_tot[1] / cnt : __builtin_nan("");
        if (a.final_pass) a.n_used[0] = (int32_t)cnt;
    }
    if (a.final_pass) return;
    const int e = blockIdx.x * kGmmThreads + tid;
    if (!any) {                                                    // nothing to fit: the parameters stay as given
        if (blockIdx.x == 0 && tid < K) a.w_out[tid] = a.w_in[tid];
        if (e < K * nz) { a.m_out[e] = a.m_in[e]; a.s_out[e] = a.s_in[e]; }
        return;
    }
    const double tot = s_tot[0];
    if (blockIdx.x == 0 && tid < K) a.w_out[tid] = (float)(s_R[tid] / tot);
    if (e >= K * nz) return;
    const double R = s_R[e / nz];
    const float m = a.m_in[e], s = a.s_in[e];
    if (R < 1e-8) { a.m_out[e] = m; a.s_out[e] = s; return; }      // a dead component keeps its place and its spread
    double s1 = 0.0, s2 = 0.0;
    const double* p1 = a.part + 2 + K + e;
    const double* p2 = p1 + (size_t)K * nz;
#pragma unroll 8
    for (int sl = 0; sl < ns; ++sl) { s1 += p1[sl * stride]; s2 += p2[sl * stride]; }
    const double d = s1 / R;
    double var = s2 / R - d * d;
    if (var < (double)a.var_floor) var = (double)a.var_floor;
    a.m_out[e] = (float)((double)m + d);
    a.s_out[e] = (float)log(var);
}

}  // namespace

void launch_gmm_estep(const GmmArgs& a, hipStream_t s) {
    const size_t lds = gmm_lds_bytes(a.K, a.nz);
    auto go = [&](auto kernel) {
        allow_max_lds(kernel);
        launch_kernel(kernel, dim3((unsigned)a.n_slices), dim3(kGmmThreads), lds, s, a);
    };
    if (a.want_stats == 0) go(k_gmm_estep<0>);
    else if (a.want_stats == 1) go(k_gmm_estep<1>);
    else go(k_gmm_estep<2>);
}

void launch_gmm_mstep(const GmmArgs& a, hipStream_t s) {
    const unsigned blocks = a.final_pass ? 1u : (unsigned)((a.K * a.nz + kGmmThreads - 1) / kGmmThreads);
    launch_kernel(k_gmm_mstep, dim3(blocks), dim3(kGmmThreads), 0, s, a);
}

}  // namespace avae
