// Cross-modal retrieval kernels of libavae (gfx950): fused latent distance + top-k (avae_latent_topk in include/avae.h; the plan,
// the list entry and the launch shapes: avae_retrieve.h).  The reference's search cost is a distance of two
// latent codes evaluated one row at a time on the host (baxter_vae_assoc_writer.py:164-166); here the rows x gallery_rows matrix
// of distances lives in registers only.
#include "avae_device.h"
#include "avae_retrieve.h"

namespace avae {

namespace {

// Every float operation below is the one written: the value of a pair must not depend on which instantiation, tile or lane
// formed it, so nothing is left to the contraction pass.  (The distance itself: latent_dist_step, avae_latent_common.h.)
#pragma clang fp contract(off)

// (order key of the distance) << 32 | index: unsigned order == (isnan, dist, index) ascending.  -0.0f cannot come out of
// latent_dist_finish (the addends are squares and products of equal signs, the sum starts from +0.0f); adding +0.0f maps it to +0.0f anyway.
__device__ __forceinline__ unsigned long long topk_entry(float dist, unsigned index) {
    unsigned b = __float_as_uint(dist + 0.0f);
    if (dist != dist) b = 0x7fc00000u;
    const unsigned key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)key << 32) | index;
}
__device__ __forceinline__ float topk_entry_dist(unsigned long long e) {
    const unsigned key = (unsigned)(e >> 32);
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}
// The filter value of a list whose last entry is e: candidates pass with !(dist >= filter).  A list that is not full, or whose
// k-th entry is a NaN, lets everything through (the exact comparison of the entries decides).
__device__ __forceinline__ float topk_filter(unsigned long long e) {
    return (unsigned)(e >> 32) >= 0xffc00000u ? __builtin_nanf("") : topk_entry_dist(e);
}

// grid (query tiles, gallery splits), kTopkThreads threads as 16 (ty: 4 queries each) x 32 (tx: 2 gallery rows each); wave w holds
// ty = 2w, 2w + 1, i.e. queries [8w, 8w + 8) of the tile, whose lists and filter values only that wave touches.
template <int METRIC>
__global__ void __launch_bounds__(kTopkThreads) k_latent_topk(TopkArgs a) {
    constexpr int TQ = kTopkQueryTile, TG = kTopkGalleryTile, LQ = kTopkQueryLd, LG = kTopkGalleryLd, SL = kTopkStashLd;
    constexpr int NA = METRIC == AVAE_METRIC_L2 ? 1 : 3;          // LDS images per side: mu (, v, iv)
    constexpr int PER = TG * kTopkMaxNz / kTopkThreads;            // staged elements per thread and tile, at most (8)
    static_assert(TQ == TG && PER * kTopkThreads == TG * kTopkMaxNz, "one staging pattern for both sides");
    extern __shared__ __attribute__((aligned(16))) unsigned char topk_lds[];
    const int nz = a.nz, k = a.k;
    unsigned long long* list = reinterpret_cast<unsigned long long*>(topk_lds);          // [k][TQ]
    float* filt = reinterpret_cast<float*>(list + (size_t)k * TQ);                        // [TQ]
    float* stash_all = filt + TQ;                                                         // [waves][TG][SL]
    float* qi_m = stash_all + (kTopkThreads / 64) * TG * SL;                              // [nz][LQ] x NA
    float* gi_m = qi_m + NA * nz * LQ;                                                    // [nz][LG] x NA
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5, wave = tid >> 6, lane = tid & 63;
    float* stash = stash_all + wave * TG * SL;
    const long long q0 = (long long)blockIdx.x * TQ;
    const int nq = (int)min((long long)TQ, a.rows - q0);           // valid queries of the tile (>= 1)
    const int n_tiles = (int)(((long long)a.gallery_rows + TG - 1) / TG);
    const int t_lo = blockIdx.y * a.tiles_per_split, t_hi = min(n_tiles, t_lo + a.tiles_per_split);
    const int n_el = TG * nz;                                      // elements of a full tile, row-major as in memory

    // where element e = tid + r * kTopkThreads of a tile (row e / nz, dimension e % nz) goes in an image of leading dimension ld
    int row_of[PER], dim_of[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int e = tid + r * kTopkThreads;
        row_of[r] = e / nz; dim_of[r] = e - row_of[r] * nz;
    }
    // lists start empty, filters open
    for (int e = tid; e < k * TQ; e += kTopkThreads) list[e] = kTopkEmpty;
    if (tid < TQ) filt[tid] = __builtin_nanf("");
    // the query tile: resident for the whole slice; rows past the end are zeros (finite arithmetic, results never used)
    {
        const float* qm = a.q_mu + q0 * nz;
        const float* ql = METRIC == AVAE_METRIC_L2 ? nullptr : a.q_lv + q0 * nz;
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int e = tid + r * kTopkThreads;
            if (e < n_el) {
                const bool in = e < nq * nz;
                const int o = dim_of[r] * LQ + row_of[r];
                qi_m[o] = in ? qm[e] : 0.0f;
                if (METRIC != AVAE_METRIC_L2) {
                    const float lv = in ? ql[e] : 0.0f;
                    qi_m[nz * LQ + o] = expf(lv);
                    qi_m[2 * nz * LQ + o] = expf(-lv);
                }
            }
        }
    }
    float pm[PER], pl[PER];                                         // the next gallery tile on its way from memory
    auto fetch = [&](int t) {
        const long long g0 = (long long)t * TG;
        const int ng = (int)min((long long)TG, a.gallery_rows - g0);
        const float* gm = a.g_mu + g0 * nz;
        const float* gl = METRIC == AVAE_METRIC_L2 ? nullptr : a.g_lv + g0 * nz;
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int e = tid + r * kTopkThreads;
            const bool in = e < ng * nz;
            pm[r] = in ? gm[e] : 0.0f;
            pl[r] = (METRIC != AVAE_METRIC_L2 && in) ? gl[e] : 0.0f;
        }
    };
    if (t_lo < t_hi) fetch(t_lo);
    for (int t = t_lo; t < t_hi; ++t) {
        __syncthreads();                                            // the previous tile's readers are done (first pass: the set-up stores)
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int e = tid + r * kTopkThreads;
            if (e < n_el) {
                const int o = dim_of[r] * LG + row_of[r];
                gi_m[o] = pm[r];
                if (METRIC != AVAE_METRIC_L2) {
                    gi_m[nz * LG + o] = expf(pl[r]);
                    gi_m[2 * nz * LG + o] = expf(-pl[r]);
                }
            }
        }
        __syncthreads();
        if (t + 1 < t_hi) fetch(t + 1);

        float acc[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) { acc[i][0] = 0.0f; acc[i][1] = 0.0f; }
#pragma unroll 4
        for (int j = 0; j < nz; ++j) {
            const float4 mq = *reinterpret_cast<const float4*>(qi_m + j * LQ + 4 * ty);
            const float2 mg = *reinterpret_cast<const float2*>(gi_m + j * LG + 2 * tx);
            float4 vq = mq, iq = mq;
            float2 vg = mg, ig = mg;
            if (METRIC != AVAE_METRIC_L2) {
                vq = *reinterpret_cast<const float4*>(qi_m + (nz + j) * LQ + 4 * ty);
                iq = *reinterpret_cast<const float4*>(qi_m + (2 * nz + j) * LQ + 4 * ty);
                vg = *reinterpret_cast<const float2*>(gi_m + (nz + j) * LG + 2 * tx);
                ig = *reinterpret_cast<const float2*>(gi_m + (2 * nz + j) * LG + 2 * tx);
            }
            const float mqa[4] = {mq.x, mq.y, mq.z, mq.w}, vqa[4] = {vq.x, vq.y, vq.z, vq.w}, iqa[4] = {iq.x, iq.y, iq.z, iq.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[i][0] = latent_dist_step<METRIC>(acc[i][0], mqa[i], vqa[i], iqa[i], mg.x, vg.x, ig.x);
                acc[i][1] = latent_dist_step<METRIC>(acc[i][1], mqa[i], vqa[i], iqa[i], mg.y, vg.y, ig.y);
            }
        }
        // selection.  Almost every candidate fails its query's filter, and then the wave does nothing more for this tile.
        const long long g0 = (long long)t * TG;
        const int ng = (int)min((long long)TG, a.gallery_rows - g0);
        const float4 f4 = *reinterpret_cast<const float4*>(filt + 4 * ty);
        const float fa[4] = {f4.x, f4.y, f4.z, f4.w};
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                acc[i][c] = latent_dist_finish<METRIC>(acc[i][c]);
                any = any || (4 * ty + i < nq && 2 * tx + c < ng && !(acc[i][c] >= fa[i]));
            }
        }
        if (__ballot(any) != 0ull) {                               // (the same in every lane of the wave)
            const int qw = 4 * (ty & 1);                            // this thread's first query among the wave's 8
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                stash[(2 * tx) * SL + qw + i] = acc[i][0];
                stash[(2 * tx + 1) * SL + qw + i] = acc[i][1];
            }
            // the wave's own stores, read back by other lanes of the same wave: the LDS keeps a wave's accesses in order
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const int q = 8 * wave + lane;                          // lanes 0..7: one query each
            if (lane < 8 && q < nq) {
                float f = filt[q];
                unsigned long long last = list[(k - 1) * TQ + q];
                for (int c = 0; c < ng; ++c) {
                    const float d = stash[c * SL + lane];
                    if (d >= f) continue;
                    const unsigned long long e = topk_entry(d, (unsigned)(g0 + c));
                    if (e >= last) continue;
                    int s = k - 1;                                  // sorted insertion from the end; the old last entry drops out
                    for (; s > 0; --s) {
                        const unsigned long long prev = list[(s - 1) * TQ + q];
                        if (prev < e) break;
                        list[s * TQ + q] = prev;
                    }
                    list[s * TQ + q] = e;
                    last = list[(k - 1) * TQ + q];
                    f = topk_filter(last);
                }
                filt[q] = f;
            }
        }
    }
    __syncthreads();
    // the tile's lists -> part[query][split][k]
    for (int e = tid; e < nq * k; e += kTopkThreads) {
        const int q = e / k, s = e - q * k;
        a.part[((size_t)(q0 + q) * a.n_splits + blockIdx.y) * k + s] = list[s * TQ + q];
    }
}

// One wave64 per query: lane l holds the heads of the lists of splits l, l + 64, ... (at most 4); k times the smallest head of all
// goes out and its list moves on.  Entries are distinct (they carry their index) except the empty ones, which end every list.
__global__ void __launch_bounds__(256) k_latent_topk_merge(TopkArgs a) {
    constexpr int H = kTopkMaxSplits / 64;
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.rows) return;
    const int k = a.k, ns = a.n_splits;
    const unsigned long long* base = a.part + (size_t)q * ns * k;
    unsigned long long head[H];
    int pos[H];
#pragma unroll
    for (int r = 0; r < H; ++r) {
        const int sp = lane + 64 * r;
        pos[r] = 0;
        head[r] = sp < ns ? base[(size_t)sp * k] : kTopkEmpty;
    }
    unsigned long long mine = kTopkEmpty;                           // lane s keeps output s
    for (int s = 0; s < k; ++s) {
        unsigned long long m = head[0];
#pragma unroll
        for (int r = 1; r < H; ++r) m = head[r] < m ? head[r] : m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned lo = __shfl_xor((unsigned)m, o), hi = __shfl_xor((unsigned)(m >> 32), o);
            const unsigned long long other = ((unsigned long long)hi << 32) | lo;
            m = other < m ? other : m;
        }
        if (lane == s) mine = m;
        if (m == kTopkEmpty) break;                                 // every list is exhausted: the rest stays empty
#pragma unroll
        for (int r = 0; r < H; ++r) {
            if (head[r] == m) {
                const int sp = lane + 64 * r;
                pos[r] += 1;
                head[r] = pos[r] < k ? base[(size_t)sp * k + pos[r]] : kTopkEmpty;
            }
        }
    }
    if (lane < k) {
        const bool empty = mine == kTopkEmpty;
        if (a.index) a.index[(size_t)q * k + lane] = empty ? -1 : (int)(unsigned)mine;
        if (a.dist) a.dist[(size_t)q * k + lane] = empty ? __builtin_inff() : topk_entry_dist(mine);
    }
}

}  // namespace

void launch_latent_topk(const TopkArgs& a, hipStream_t s) {
    const size_t lds = topk_lds_bytes(a.nz, a.k, a.metric);
    const dim3 grid((unsigned)((a.rows + kTopkQueryTile - 1) / kTopkQueryTile), (unsigned)a.n_splits);
    auto go = [&](auto kernel) {
        allow_max_lds(kernel);
        launch_kernel(kernel, grid, dim3(kTopkThreads), lds, s, a);
    };
    if (a.metric == AVAE_METRIC_L2) go(k_latent_topk<AVAE_METRIC_L2>);
    else go(k_latent_topk<AVAE_METRIC_SYMKL>);
}

void launch_latent_topk_merge(const TopkArgs& a, hipStream_t s) {
    launch_kernel(k_latent_topk_merge, dim3((unsigned)((a.rows + 3) / 4)), dim3(256), 0, s, a);
}

}  // namespace avae
