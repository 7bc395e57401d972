// t-SNE kernels of libavae (gfx950): perplexity calibration and the gradient-descent loop of a 2-D map of the posteriors
// (avae_embed_calibrate / avae_embed_iterate in include/avae.h; the plan, the scratch and the launch shapes: avae_embed.h;
// DESIGN.md section 22).  The rows x rows matrices of distances and affinities live in registers only.
#include "avae_device.h"
#include "avae_embed.h"

namespace avae {

namespace {

// Every float operation below is the one written (a fused multiply-add only where __builtin_fmaf says so): the distance of a pair
// must have the same bits in the calibration and in every force pass, whichever tile, split or lane formed it.
#pragma clang fp contract(off)

constexpr int T = kEmbedTile, LD = kEmbedLd, PER = kEmbedTile * kEmbedMaxNz / kEmbedThreads;   // staged elements per thread and tile, at most (16)
static_assert(PER * kEmbedThreads == T * kEmbedMaxNz && kEmbedThreads == 256 && T == 64, "16 x 16 threads, 4 x 4 pairs each");
// per-row words of a tile side in LDS, [word][64]
enum { W_BETA = 0, W_SHIFT = 1, W_C = 2, W_Y0 = 3, W_Y1 = 4, W_USED = 5, W_LO = 6, W_HI = 7 };

// The distance of a pair is avae_latent_topk's (include/avae.h): the same latent_dist_step / latent_dist_finish (avae_latent_common.h).

// The tile of rows [r0, r0 + 64) on its way from memory: element e = tid + i * 256 of the tile, row-major as in memory.  Rows past
// the end read as zeros (finite arithmetic, selected away by their used byte).
template <int METRIC>
__device__ __forceinline__ void embed_fetch(const EmbedArgs& a, long long r0, int tid, float (&pm)[PER], float (&pl)[PER]) {
    const int cnt = (int)min((long long)T, (long long)a.rows - r0) * a.nz;
    const float* m = a.mu + (size_t)r0 * a.nz;
    const float* l = METRIC == AVAE_METRIC_L2 ? nullptr : a.lv + (size_t)r0 * a.nz;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int e = tid + i * kEmbedThreads;
        const bool in = e < cnt;
        pm[i] = in ? m[e] : 0.0f;
        pl[i] = (METRIC != AVAE_METRIC_L2 && in) ? l[e] : 0.0f;
    }
}
// ... and into its LDS images [n_z][LD]: mu (, v = expf(lv), iv = expf(-lv))
template <int METRIC>
__device__ __forceinline__ void embed_store(float* img, int nz, int tid, const float (&pm)[PER], const float (&pl)[PER]) {
    const int n_el = T * nz;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int e = tid + i * kEmbedThreads;
        if (e < n_el) {
            const int row = e / nz, j = e - row * nz;
            const int o = j * LD + row;
            img[o] = pm[i];
            if (METRIC != AVAE_METRIC_L2) {
                img[nz * LD + o] = expf(pl[i]);
                img[2 * nz * LD + o] = expf(-pl[i]);
            }
        }
    }
}

// The 4 x 4 distances of rows 4 ty .. 4 ty + 3 of the row side and 4 tx .. 4 tx + 3 of the streamed side.
template <int METRIC>
__device__ __forceinline__ void embed_dist_block(const float* qi, const float* gi, int nz, int ty, int tx, float (&D)[4][4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) D[r][c] = 0.0f;
#pragma unroll 2
    for (int j = 0; j < nz; ++j) {
        const float4 mq = *reinterpret_cast<const float4*>(qi + j * LD + 4 * ty);
        const float4 mg = *reinterpret_cast<const float4*>(gi + j * LD + 4 * tx);
        float4 vq = mq, iq = mq, vg = mg, ig = mg;
        if (METRIC != AVAE_METRIC_L2) {
            vq = *reinterpret_cast<const float4*>(qi + (nz + j) * LD + 4 * ty);
            iq = *reinterpret_cast<const float4*>(qi + (2 * nz + j) * LD + 4 * ty);
            vg = *reinterpret_cast<const float4*>(gi + (nz + j) * LD + 4 * tx);
            ig = *reinterpret_cast<const float4*>(gi + (2 * nz + j) * LD + 4 * tx);
        }
        const float mqa[4] = {mq.x, mq.y, mq.z, mq.w}, vqa[4] = {vq.x, vq.y, vq.z, vq.w}, iqa[4] = {iq.x, iq.y, iq.z, iq.w};
        const float mga[4] = {mg.x, mg.y, mg.z, mg.w}, vga[4] = {vg.x, vg.y, vg.z, vg.w}, iga[4] = {ig.x, ig.y, ig.z, ig.w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) D[r][c] = latent_dist_step<METRIC>(D[r][c], mqa[r], vqa[r], iqa[r], mga[c], vga[c], iga[c]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) D[r][c] = latent_dist_finish<METRIC>(D[r][c]);
}

// The 16 threads of a row (consecutive lanes of one wave) combined by a fixed tree; every lane ends with the result.
__device__ __forceinline__ double embed_row_sum(double x) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) x = x + __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ float embed_row_min(float x) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) x = __builtin_fminf(x, __shfl_xor(x, o));
    return x;
}

// The used rows of the whole input: the blocks' counts in block order (integers: exact)
__device__ __forceinline__ int embed_used_rows(const EmbedArgs& a) {
    int f = 0;
    for (int b = 0; b < (a.rows + kEmbedScanRows - 1) / kEmbedScanRows; ++b) f += a.count[b];
    return f;
}

// grid = blocks of 256 rows, one thread per row
__global__ void __launch_bounds__(kEmbedThreads) k_embed_scan(EmbedArgs a) {
    __shared__ int s_cnt[kEmbedThreads / 64];
    const int tid = threadIdx.x;
    const long long row = (long long)blockIdx.x * kEmbedScanRows + tid;
    bool ok = row < a.rows;
    if (ok) {
        const float* m = a.mu + (size_t)row * a.nz;
        for (int j = 0; j < a.nz; ++j) ok = ok && latent_finite(m[j]);
        if (a.lv) {
            const float* l = a.lv + (size_t)row * a.nz;
            for (int j = 0; j < a.nz; ++j) ok = ok && latent_finite(l[j]);
        }
        a.used[row] = ok ? 1 : 0;
    }
    const unsigned long long m = __ballot(ok);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int c = 0;
        for (int w = 0; w < kEmbedThreads / 64; ++w) c += s_cnt[w];
        a.count[blockIdx.x] = c;
    }
}

// grid = row tiles.  Pass 0 finds the rows' minima; every further pass is one try of the search for the rows not yet finished.
template <int METRIC>
__global__ void __launch_bounds__(kEmbedThreads) k_embed_calibrate(EmbedArgs a) {
    constexpr int NA = METRIC == AVAE_METRIC_L2 ? 1 : 3;
    extern __shared__ __attribute__((aligned(16))) unsigned char embed_lds[];
    const int nz = a.nz;
    float* qi = reinterpret_cast<float*>(embed_lds);               // row side: [NA][nz][LD]
    float* gi = qi + NA * nz * LD;                                 // streamed side
    float* rs = gi + NA * nz * LD;                                 // [8][64] words of the row side
    float* cs = rs + kEmbedRowWords * T;                           // ... of the streamed side (the used word alone)
    int& s_F = reinterpret_cast<int*>(cs + W_LO * T)[0];          // (no static LDS: the dynamic part may be all of the CU's)
    int& s_left = reinterpret_cast<int*>(cs + W_LO * T)[1];
    int* r_done = reinterpret_cast<int*>(rs + W_C * T);           // (the words the force pass uses for c, y0, y1)
    int* r_tries = reinterpret_cast<int*>(rs + W_Y0 * T);
    float* r_norm = rs + W_Y1 * T;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long long r0 = (long long)blockIdx.x * T;
    const int nq = (int)min((long long)T, (long long)a.rows - r0);
    const int n_tiles = (a.rows + T - 1) / T;
    const float nanv = __builtin_nanf("");

    float pm[PER], pl[PER];
    embed_fetch<METRIC>(a, r0, tid, pm, pl);
    if (tid == 0) s_F = embed_used_rows(a);
    embed_store<METRIC>(qi, nz, tid, pm, pl);
    __syncthreads();
    const int F = s_F;
    if (tid < T) {
        const bool used = tid < nq && a.used[r0 + tid] != 0 && F >= 2;
        reinterpret_cast<int*>(rs + W_USED * T)[tid] = used ? 1 : 0;
        rs[W_BETA * T + tid] = used ? 1.0f : nanv;
        rs[W_SHIFT * T + tid] = nanv;
        rs[W_LO * T + tid] = 0.0f;                                 // 0: no lower bound yet; +Inf: no upper bound yet
        rs[W_HI * T + tid] = __builtin_inff();
        r_done[tid] = used ? 0 : 1;
        r_tries[tid] = 0;
        r_norm[tid] = nanv;
    }
    __syncthreads();
    bool okr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) okr[r] = reinterpret_cast<const int*>(rs + W_USED * T)[4 * ty + r] != 0;

    for (int pass = 0; pass <= a.max_tries; ++pass) {
        float bi[4], mi[4], mn[4];
        double S0[4], S1[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            bi[r] = rs[W_BETA * T + 4 * ty + r]; mi[r] = rs[W_SHIFT * T + 4 * ty + r];
            mn[r] = __builtin_inff(); S0[r] = 0.0; S1[r] = 0.0;
        }
        unsigned char pu = 0;                                      // the next tile's used byte, threads 0..63
        auto fetch = [&](int t) {
            const long long c0 = (long long)t * T;
            embed_fetch<METRIC>(a, c0, tid, pm, pl);
            if (tid < T) pu = c0 + tid < a.rows ? a.used[c0 + tid] : 0;
        };
        fetch(0);
        for (int t = 0; t < n_tiles; ++t) {
            const long long c0 = (long long)t * T;
            __syncthreads();                                       // the previous tile's readers are done
            embed_store<METRIC>(gi, nz, tid, pm, pl);
            if (tid < T) reinterpret_cast<int*>(cs + W_USED * T)[tid] = pu;
            __syncthreads();
            if (t + 1 < n_tiles) fetch(t + 1);
            float D[4][4];
            embed_dist_block<METRIC>(qi, gi, nz, ty, tx, D);
            bool okc[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) okc[c] = reinterpret_cast<const int*>(cs + W_USED * T)[4 * tx + c] != 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    // a pair is selected, never multiplied by 0: a skipped row's NaN stops here
                    const bool on = okr[r] && okc[c] && (r0 + 4 * ty + r) != (c0 + 4 * tx + c);
                    if (pass == 0) {
                        mn[r] = on ? __builtin_fminf(mn[r], D[r][c]) : mn[r];
                    } else {
                        const float d = D[r][c] - mi[r];
                        const float e = expf(-(bi[r] * d));
                        s0 = s0 + (on ? e : 0.0f);
                        s1 = s1 + (on ? d * e : 0.0f);
                    }
                }
                S0[r] = S0[r] + (double)s0;
                S1[r] = S1[r] + (double)s1;
            }
        }
        // the 16 threads of a row; its first one keeps the row's state
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * ty + r;
            if (pass == 0) {
                const float m = embed_row_min(mn[r]);
                if (tx == 0 && okr[r]) rs[W_SHIFT * T + row] = m;
            } else {
                const double s0 = embed_row_sum(S0[r]), s1 = embed_row_sum(S1[r]);
                if (tx == 0 && r_done[row] == 0) {
                    const float beta = bi[r];
                    const double H = log(s0) + (double)beta * s1 / s0;
                    const double diff = H - a.log_perp;
                    const int tries = r_tries[row] + 1;
                    r_tries[row] = tries;
                    if (fabs(diff) <= a.tol || tries >= a.max_tries || !(diff == diff)) {
                        r_done[row] = 1;
                        r_norm[row] = (float)s0;
                    } else if (diff > 0.0) {                       // too flat: a larger beta
                        const float hi = rs[W_HI * T + row];
                        rs[W_LO * T + row] = beta;
                        rs[W_BETA * T + row] = hi == __builtin_inff() ? __builtin_fminf(beta * 2.0f, kEmbedBetaMax) : (beta + hi) * 0.5f;
                    } else {
                        const float lo = rs[W_LO * T + row];
                        rs[W_HI * T + row] = beta;
                        rs[W_BETA * T + row] = lo == 0.0f ? __builtin_fmaxf(beta * 0.5f, kEmbedBetaMin) : (beta + lo) * 0.5f;
                    }
                }
            }
        }
        __syncthreads();
        if (tid < 64) {
            const unsigned long long left = __ballot(r_done[tid] == 0);
            if (tid == 0) s_left = left != 0ull ? 1 : 0;
        }
        __syncthreads();
        if (s_left == 0) break;
    }
    if (tid < nq) {
        const bool used = reinterpret_cast<const int*>(rs + W_USED * T)[tid] != 0;
        a.beta[r0 + tid] = rs[W_BETA * T + tid];
        a.shift[r0 + tid] = used ? rs[W_SHIFT * T + tid] : nanv;
        a.norm[r0 + tid] = r_norm[tid];
        a.tries[r0 + tid] = r_tries[tid];
    }
    if (blockIdx.x == 0 && tid == 0) a.n_used[0] = F;
}

// grid (row tiles, splits).  PLOGP: also the sum of p log p per row, the part of the KL that does not depend on Y.
template <int METRIC, bool PLOGP>
__global__ void __launch_bounds__(kEmbedThreads) k_embed_forces(EmbedArgs a) {
    constexpr int NA = METRIC == AVAE_METRIC_L2 ? 1 : 3, NS = kEmbedParts + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char embed_lds[];
    const int nz = a.nz;
    float* qi = reinterpret_cast<float*>(embed_lds);
    float* gi = qi + NA * nz * LD;
    float* rs = gi + NA * nz * LD;
    float* cs = rs + kEmbedRowWords * T;
    int& s_F = reinterpret_cast<int*>(cs + W_LO * T)[0];          // (no static LDS: the dynamic part may be all of the CU's)
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long long r0 = (long long)blockIdx.x * T;
    const int n_tiles = (a.rows + T - 1) / T;
    const int t_lo = blockIdx.y * a.tiles_per_split, t_hi = min(n_tiles, t_lo + a.tiles_per_split);

    float pm[PER], pl[PER];
    float ps[6];                                                   // a tile side's per-row words, threads 0..63
    if (tid == 0) s_F = embed_used_rows(a);
    __syncthreads();
    const float two_f = 2.0f * (float)s_F;
    auto fetch = [&](long long c0) {
        embed_fetch<METRIC>(a, c0, tid, pm, pl);
        if (tid < T) {
            const long long row = c0 + tid;
            const bool in = row < a.rows;
            const bool used = in && a.used[row] != 0;
            ps[W_BETA] = in ? a.beta[row] : 0.0f;
            ps[W_SHIFT] = in ? a.shift[row] : 0.0f;
            ps[W_C] = in ? 1.0f / (two_f * a.norm[row]) : 0.0f;    // c = 1 / (2 F S0)
            ps[W_Y0] = in ? a.y[2 * row] : 0.0f;
            ps[W_Y1] = in ? a.y[2 * row + 1] : 0.0f;
            ps[W_USED] = __int_as_float(used ? 1 : 0);
        }
    };
    auto store = [&](float* img, float* words) {
        embed_store<METRIC>(img, nz, tid, pm, pl);
        if (tid < T) {
#pragma unroll
            for (int w = 0; w < 6; ++w) words[w * T + tid] = ps[w];
        }
    };
    fetch(r0);
    store(qi, rs);
    __syncthreads();
    float bi[4], mi[4], ci[4], y0i[4], y1i[4];
    bool okr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * ty + r;
        bi[r] = rs[W_BETA * T + row]; mi[r] = rs[W_SHIFT * T + row]; ci[r] = rs[W_C * T + row];
        y0i[r] = rs[W_Y0 * T + row]; y1i[r] = rs[W_Y1 * T + row];
        okr[r] = __float_as_int(rs[W_USED * T + row]) != 0;
    }
    double acc[4][NS];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < NS; ++q) acc[r][q] = 0.0;

    if (t_lo < t_hi) fetch((long long)t_lo * T);
    for (int t = t_lo; t < t_hi; ++t) {
        const long long c0 = (long long)t * T;
        __syncthreads();                                           // the previous tile's readers are done
        store(gi, cs);
        __syncthreads();
        if (t + 1 < t_hi) fetch((long long)(t + 1) * T);
        float D[4][4];
        embed_dist_block<METRIC>(qi, gi, nz, ty, tx, D);
        float bj[4], mj[4], cj[4], y0j[4], y1j[4];
        bool okc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int col = 4 * tx + c;
            bj[c] = cs[W_BETA * T + col]; mj[c] = cs[W_SHIFT * T + col]; cj[c] = cs[W_C * T + col];
            y0j[c] = cs[W_Y0 * T + col]; y1j[c] = cs[W_Y1 * T + col];
            okc[c] = __float_as_int(cs[W_USED * T + col]) != 0;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float s[NS];
#pragma unroll
            for (int q = 0; q < NS; ++q) s[q] = 0.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                // a pair is selected, never multiplied by 0: nothing a skipped row holds gets past these three selects
                const bool on = okr[r] && okc[c] && (r0 + 4 * ty + r) != (c0 + 4 * tx + c);
                const float eij = expf(-(bi[r] * (D[r][c] - mi[r])));
                const float eji = expf(-(bj[c] * (D[r][c] - mj[c])));
                const float pr = eij * ci[r] + eji * cj[c];        // (two products and a sum: p_ij and p_ji are the same bits)
                const float p = on ? pr : 0.0f;
                const float d0 = on ? y0i[r] - y0j[c] : 0.0f, d1 = on ? y1i[r] - y1j[c] : 0.0f;
                const float q = __builtin_fmaf(d1, d1, __builtin_fmaf(d0, d0, 1.0f));
                const float w = on ? 1.0f / q : 0.0f;
                const float pw = p * w, ww = w * w;
                s[0] = s[0] + pw * d0; s[1] = s[1] + pw * d1;
                s[2] = s[2] + ww * d0; s[3] = s[3] + ww * d1;
                s[4] = s[4] + w;
                s[5] = s[5] + (p > 0.0f ? p * logf(q) : 0.0f);    // - p log w
                if (PLOGP) s[6] = s[6] + (p > 0.0f ? p * logf(p) : 0.0f);
            }
#pragma unroll
            for (int q = 0; q < NS; ++q) acc[r][q] = acc[r][q] + (double)s[q];
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long row = r0 + 4 * ty + r;
        const size_t slot = (size_t)row * a.n_splits + blockIdx.y;
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            if (q == kEmbedParts && !PLOGP) continue;
            const double v = embed_row_sum(acc[r][q]);
            if (tx == 0 && row < a.rows) {
                if (q < kEmbedParts) a.part[(size_t)q * a.part_stride + slot] = v;
                else a.plogp[slot] = v;
            }
        }
    }
}

// grid = blocks of 256 rows.  Every block forms Z, the KL and (evaluating, centring) the mean of y for itself: thread t adds the
// rows t, t + 256, ..., each row's splits in split order, then thread 0 the 256 sums in thread order.
__global__ void __launch_bounds__(kEmbedThreads) k_embed_update(EmbedArgs a) {
    __shared__ double s_sum[4][kEmbedThreads];
    __shared__ double s_tot[4];
    __shared__ int s_F;
    const int tid = threadIdx.x, ns = a.n_splits;
    const size_t stride = a.part_stride;
    const bool want_mean = a.evaluate && a.center && blockIdx.x == 0;
    double z = 0.0, k = 0.0, m0 = 0.0, m1 = 0.0;
    for (long long row = tid; row < a.rows; row += kEmbedThreads) {
        const size_t s0 = (size_t)row * ns;
        for (int s = 0; s < ns; ++s) {
            z = z + a.part[4 * stride + s0 + s];
            k = k + a.part[5 * stride + s0 + s];
            k = k + a.plogp[s0 + s];
        }
        if (want_mean && a.used[row]) { m0 = m0 + (double)a.y[2 * row]; m1 = m1 + (double)a.y[2 * row + 1]; }
    }
    s_sum[0][tid] = z; s_sum[1][tid] = k; s_sum[2][tid] = m0; s_sum[3][tid] = m1;
    if (tid == 64) s_F = embed_used_rows(a);
    __syncthreads();
    if (tid < 4) {
        double t = 0.0;
        for (int i = 0; i < kEmbedThreads; ++i) t = t + s_sum[tid][i];
        s_tot[tid] = t;
    }
    __syncthreads();
    const int F = s_F;
    const bool any = F >= 2;                                       // fewer than two used rows: nothing to embed
    const double Z = s_tot[0];
    if (blockIdx.x == 0 && tid == 0) {
        a.kl[0] = any ? s_tot[1] + log(Z) : __builtin_nan("");
        if (want_mean) { a.mean[0] = any ? s_tot[2] / (double)F : 0.0; a.mean[1] = any ? s_tot[3] / (double)F : 0.0; }
    }
    const long long row = (long long)blockIdx.x * kEmbedScanRows + tid;
    if (row >= a.rows) return;
    const bool used = a.used[row] != 0;
    double A[2] = {0.0, 0.0}, R[2] = {0.0, 0.0};
    const size_t s0 = (size_t)row * ns;
    for (int s = 0; s < ns; ++s) {
        A[0] = A[0] + a.part[0 * stride + s0 + s]; A[1] = A[1] + a.part[1 * stride + s0 + s];
        R[0] = R[0] + a.part[2 * stride + s0 + s]; R[1] = R[1] + a.part[3 * stride + s0 + s];
    }
    const float nanv = __builtin_nanf("");
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const size_t i = 2 * (size_t)row + c;
        const double g = 4.0 * ((double)a.alpha * A[c] - R[c] / Z);
        if (a.grad) a.grad[i] = used && any ? (float)g : nanv;
        if (a.evaluate) continue;
        if (!used) { a.y[i] = nanv; a.vel[i] = nanv; a.gain[i] = nanv; continue; }
        if (!any) continue;
        const float v = a.vel[i], gn = a.gain[i], y = a.y[i];
        const double g64 = ((g > 0.0) != (v > 0.0f)) ? (double)gn + 0.2 : (double)gn * 0.8;
        const float gn32 = (float)fmax(g64, 0.01);
        const float v32 = (float)((double)a.mom * (double)v - ((double)a.lr * (double)gn32) * g);
        a.gain[i] = gn32;
        a.vel[i] = v32;
        a.y[i] = (float)((double)y + (double)v32);
    }
}

// grid = blocks of 256 rows, one thread per row
__global__ void __launch_bounds__(kEmbedThreads) k_embed_center(EmbedArgs a) {
    const long long row = (long long)blockIdx.x * kEmbedScanRows + threadIdx.x;
    if (row >= a.rows || !a.used[row]) return;
    a.y[2 * row] = (float)((double)a.y[2 * row] - a.mean[0]);
    a.y[2 * row + 1] = (float)((double)a.y[2 * row + 1] - a.mean[1]);
}

template <typename K> void embed_tiled(K kernel, dim3 grid, const EmbedArgs& a, hipStream_t s) {
    allow_max_lds(kernel);
    launch_kernel(kernel, grid, dim3(kEmbedThreads), embed_lds_bytes(a.nz, a.metric), s, a);
}

unsigned embed_row_blocks(const EmbedArgs& a) { return (unsigned)((a.rows + kEmbedScanRows - 1) / kEmbedScanRows); }
unsigned embed_row_tiles(const EmbedArgs& a) { return (unsigned)((a.rows + kEmbedTile - 1) / kEmbedTile); }

}  // namespace

void launch_embed_scan(const EmbedArgs& a, hipStream_t s) {
    launch_kernel(k_embed_scan, dim3(embed_row_blocks(a)), dim3(kEmbedThreads), 0, s, a);
}

void launch_embed_calibrate(const EmbedArgs& a, hipStream_t s) {
    if (a.metric == AVAE_METRIC_L2) embed_tiled(k_embed_calibrate<AVAE_METRIC_L2>, dim3(embed_row_tiles(a)), a, s);
    else embed_tiled(k_embed_calibrate<AVAE_METRIC_SYMKL>, dim3(embed_row_tiles(a)), a, s);
}

void launch_embed_forces(const EmbedArgs& a, hipStream_t s) {
    const dim3 grid(embed_row_tiles(a), (unsigned)a.n_splits);
    if (a.metric == AVAE_METRIC_L2) {
        if (a.first_pass) embed_tiled(k_embed_forces<AVAE_METRIC_L2, true>, grid, a, s);
        else embed_tiled(k_embed_forces<AVAE_METRIC_L2, false>, grid, a, s);
    } else {
        if (a.first_pass) embed_tiled(k_embed_forces<AVAE_METRIC_SYMKL, true>, grid, a, s);
        else embed_tiled(k_embed_forces<AVAE_METRIC_SYMKL, false>, grid, a, s);
    }
}

void launch_embed_update(const EmbedArgs& a, hipStream_t s) {
    launch_kernel(k_embed_update, dim3(embed_row_blocks(a)), dim3(kEmbedThreads), 0, s, a);
}

void launch_embed_center(const EmbedArgs& a, hipStream_t s) {
    launch_kernel(k_embed_center, dim3(embed_row_blocks(a)), dim3(kEmbedThreads), 0, s, a);
}

}  // namespace avae
