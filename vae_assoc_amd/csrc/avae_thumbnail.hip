// Letter thumbnail kernels (avae_thumbnail.h, include/avae.h): k_ink_box, k_thumbnail.
#include <limits.h>
#include "avae_device.h"
#include "avae_thumbnail.h"

namespace avae {

namespace {

// a pixel's bytes as one word (byte 0 lowest), loaded one by one: any address, nothing beyond the pixel
template <int C> __device__ __forceinline__ uint32_t load_pixel(const uint8_t* p) {
    uint32_t px = p[0];
    if (C > 1) px |= (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    return px;
}

// grey value of a pixel word; k0 / k2 weigh its first / third byte (4899 / 1868 for rgb, swapped for bgr)
template <int C> __device__ __forceinline__ int grey_of(uint32_t px, uint32_t k0, uint32_t k2) {
    if (C == 1) return (int)(px & 255u);
    return (int)((k0 * (px & 255u) + 9617u * ((px >> 8) & 255u) + k2 * ((px >> 16) & 255u) + 8192u) >> 14);
}

struct BoxAcc {
    int x0, x1, cnt;
    __device__ __forceinline__ void add(int col) { x0 = min(x0, col); x1 = max(x1, col); ++cnt; }
};

// ------------------------------------------------------------------------------------------------ bounding box of the ink
template <int C>
__global__ __launch_bounds__(kThumbThreads) void k_ink_box(const ThumbArgs a) {
    __shared__ int red_s[kThumbThreads / 64][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long frame = blockIdx.x / a.slabs;
    const int slab = (int)(blockIdx.x - frame * a.slabs);
    const int ya = slab * a.slab_rows, yb = min(a.Hf, ya + a.slab_rows);
    const uint32_t k0 = a.bgr ? 1868u : 4899u, k2 = a.bgr ? 4899u : 1868u;
    const int level = thumb_ink_level(a.threshold, a.invert != 0);
    const bool inv = a.invert != 0;
    const int nbytes = a.Wf * C;
    const uint8_t* fr = a.frames + frame * a.frame_stride;
    BoxAcc acc = {INT_MAX, -1, 0};
    int y0 = INT_MAX, y1 = -1;
    for (int y = ya + wave; y < yb; y += kThumbThreads / 64) {
        const uint8_t* lo = fr + (long long)y * a.row_stride;
        const int lead = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(lo) & 15u)) & 15u);   // bytes ahead of the first 16-byte line
        const int nfull = nbytes >= lead + 16 ? (nbytes - lead) >> 4 : 0;                           // whole chunks inside the row
        const int before = acc.cnt;
        for (int ch = lane; ch < nfull; ch += 64) {
            const int off = lead + 16 * ch;
            const uint4 q = *reinterpret_cast<const uint4*>(lo + off);
            if constexpr (C == 1) {
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
                uint32_t mask = 0;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int v = (int)((w[j >> 2] >> (8 * (j & 3))) & 255u);
                    mask |= (uint32_t)((v > level) != inv) << j;
                }
                if (mask) {
                    acc.cnt += __popc(mask);
                    acc.x0 = min(acc.x0, off + (__ffs((int)mask) - 1));
                    acc.x1 = max(acc.x1, off + 31 - __clz((int)mask));
                }
            } else {
                // the pixels that start in this chunk may end in the next 4 bytes
                const int rest = nbytes - (off + 16);
                uint32_t w4 = 0;
                if (rest >= 4) {
                    w4 = *reinterpret_cast<const uint32_t*>(lo + off + 16);
                } else {
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        if (j < rest) w4 |= (uint32_t)lo[off + 16 + j] << (8 * j);
                }
                const uint32_t w[5] = {q.x, q.y, q.z, q.w, w4};
                const int first = (C - off % C) % C;            // the chunk's first byte that starts a pixel
                const int px0 = (off + first) / C;
                constexpr int K = C == 3 ? 6 : 4;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int base = C * k, i = base >> 2, sh = base & 3;
                    const uint64_t two = (uint64_t)w[i] | (uint64_t)w[i + 1] << 32;
                    const uint32_t px = (uint32_t)(two >> (8 * (sh + first)));      // sh + first <= 5: the pixel's 3 bytes are inside
                    const int v = grey_of<C>(px, k0, k2);
                    if (base + first < 16 && (v > level) != inv) acc.add(px0 + k);
                }
            }
        }
        // the pixels that start ahead of the first or behind the last whole chunk (every pixel of a row without one)
        const int head = nfull ? (lead + C - 1) / C : a.Wf;
        const int tail0 = nfull ? (lead + 16 * nfull + C - 1) / C : a.Wf;
        const int narrow = head + (a.Wf - tail0);
        for (int n = lane; n < narrow; n += 64) {
            const int col = n < head ? n : tail0 + (n - head);
            const int v = grey_of<C>(load_pixel<C>(lo + (size_t)col * C), k0, k2);
            if ((v > level) != inv) acc.add(col);
        }
        if (acc.cnt != before) { y0 = min(y0, y); y1 = max(y1, y); }
    }
    int x0 = acc.x0, x1 = acc.x1, cnt = acc.cnt;
    for (int o = 32; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o)); x1 = max(x1, __shfl_xor(x1, o));
        y0 = min(y0, __shfl_xor(y0, o)); y1 = max(y1, __shfl_xor(y1, o));
        cnt += __shfl_xor(cnt, o);
    }
    if (lane == 0) { red_s[wave][0] = x0; red_s[wave][1] = x1; red_s[wave][2] = y0; red_s[wave][3] = y1; red_s[wave][4] = cnt; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < kThumbThreads / 64; ++v) {
            x0 = min(x0, red_s[v][0]); x1 = max(x1, red_s[v][1]); y0 = min(y0, red_s[v][2]); y1 = max(y1, red_s[v][3]);
            cnt += red_s[v][4];
        }
        int4* rec = reinterpret_cast<int4*>(a.records + ((size_t)frame * a.slabs + slab) * kThumbRecordInts);
        rec[0] = make_int4(x0, x1, y0, y1);
        rec[1] = make_int4(cnt, 0, 0, 0);
    }
}

// ------------------------------------------------------------------------------------------------ window and area mean
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
    const int lo = __shfl_xor((int)(unsigned)v, o), hi = __shfl_xor((int)(unsigned)(v >> 32), o);
    return (unsigned long long)(unsigned)lo | (unsigned long long)(unsigned)hi << 32;
}

template <int C>
__global__ __launch_bounds__(kThumbThreads) void k_thumbnail(const ThumbArgs a) {
    __shared__ uint32_t col_s[kThumbMaxFrame];
    const int tid = threadIdx.x, Ho = a.size;
    const long long frame = blockIdx.x / Ho;
    const int i = (int)(blockIdx.x - frame * Ho);
    const int4* rec = reinterpret_cast<const int4*>(a.records + (size_t)frame * a.slabs * kThumbRecordInts);
    int x0 = INT_MAX, x1 = -1, y0 = INT_MAX, y1 = -1, cnt = 0;
    for (int s = 0; s < a.slabs; ++s) {
        const int4 r = rec[2 * s];
        x0 = min(x0, r.x); x1 = max(x1, r.y); y0 = min(y0, r.z); y1 = max(y1, r.w);
        cnt += rec[2 * s + 1].x;
    }
    const bool blank = cnt == 0;
    const int x = blank ? 0 : x0, y = blank ? 0 : y0, w = blank ? a.Wf : x1 - x0 + 1, h = blank ? a.Hf : y1 - y0 + 1;
    const int L = max(w, h), b = 3 * L / 5, S = L + b;
    const int oy = b / 2 + (L - h) / 2, ox = b / 2 + (L - w) / 2;
    if (i == 0 && tid == 0) {
        if (a.box) { int32_t* p = a.box + frame * 4; p[0] = x; p[1] = y; p[2] = w; p[3] = h; }
        if (a.window) { int32_t* p = a.window + frame * 3; p[0] = x - ox; p[1] = y - oy; p[2] = S; }
        if (a.ink) a.ink[frame] = cnt;
    }
    if (!a.image) return;
    float* out = a.image + ((size_t)frame * Ho + i) * Ho;
    if (blank) {
        if (tid < Ho) out[tid] = 0.0f;
        return;
    }
    // column sums of the canvas rows that meet output row i, over the crop
    const uint32_t k0 = a.bgr ? 1868u : 4899u, k2 = a.bgr ? 4899u : 1868u;
    const int level = thumb_ink_level(a.threshold, a.invert != 0);
    const bool inv = a.invert != 0, binary = a.threshold >= 0;
    const int band0 = i * S, band1 = band0 + S;                             // the footprint in units of 1 / Ho of a cell
    const int ra = max(band0 / Ho - oy, 0), rb = min((band1 + Ho - 1) / Ho - oy, h);
    const uint8_t* corner = a.frames + frame * a.frame_stride + (long long)(y + ra) * a.row_stride + (size_t)x * C;
    for (int c = tid; c < w; c += kThumbThreads) {                          // at most kThumbCols columns a thread
        const uint8_t* p = corner + (size_t)c * C;
        uint32_t s = 0;
#pragma unroll 4                                                            // (four rows' loads in flight)
        for (int r = ra; r < rb; ++r, p += a.row_stride) {
            const int k = r + oy;
            const uint32_t wy = (uint32_t)(min(band1, (k + 1) * Ho) - max(band0, k * Ho));
            const int v = grey_of<C>(load_pixel<C>(p), k0, k2);
            const uint32_t g = binary ? (((v > level) != inv) ? 255u : 0u) : (uint32_t)(inv ? 255 - v : v);
            s += wy * g;
        }
        col_s[c] = s;
    }
    __syncthreads();
    // output pixel j: tpb threads add wx times the column sums, a shuffle tree joins them
    int tpb = 64;
    while (tpb * Ho > kThumbThreads) tpb >>= 1;
    const int j = tid / tpb, sub = tid & (tpb - 1);
    unsigned long long sum = 0;
    if (j < Ho) {
        const int foot0 = j * S, foot1 = foot0 + S;
        const int ca = max(foot0 / Ho - ox, 0), cb = min((foot1 + Ho - 1) / Ho - ox, w);
        for (int c = ca + sub; c < cb; c += tpb) {
            const int k = c + ox;
            const uint32_t wx = (uint32_t)(min(foot1, (k + 1) * Ho) - max(foot0, k * Ho));
            sum += (unsigned long long)wx * col_s[c];
        }
    }
    for (int o = tpb >> 1; o > 0; o >>= 1) sum += shfl_xor_u64(sum, o);
    if (j < Ho && sub == 0) out[j] = (float)((double)sum / (double)(255ull * (unsigned long long)S * (unsigned long long)S));
}

}  // namespace

void launch_ink_box(const ThumbArgs& a, long long rows, hipStream_t s) {
    const dim3 grid((unsigned)(rows * a.slabs)), block(kThumbThreads);
    switch (a.C) {
        case 1: launch_kernel(k_ink_box<1>, grid, block, 0, s, a); break;
        case 3: launch_kernel(k_ink_box<3>, grid, block, 0, s, a); break;
        default: launch_kernel(k_ink_box<4>, grid, block, 0, s, a); break;
    }
}

void launch_thumbnail(const ThumbArgs& a, long long rows, hipStream_t s) {
    const dim3 grid((unsigned)(rows * a.size)), block(kThumbThreads);
    switch (a.C) {
        case 1: launch_kernel(k_thumbnail<1>, grid, block, 0, s, a); break;
        case 3: launch_kernel(k_thumbnail<3>, grid, block, 0, s, a); break;
        default: launch_kernel(k_thumbnail<4>, grid, block, 0, s, a); break;
    }
}

}  // namespace avae
