// What the latent-space features share (DESIGN.md sections 18-23: avae_retrieve, avae_latent_stats, avae_aggpost, avae_gmm,
// avae_embed, avae_motion): the distance of two posteriors, the finite test, and the two partitions their plans are built from.
// Internal to csrc/; the plan structs, the constants and the *_scratch_bytes / *_lds_bytes functions stay in the feature headers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include "avae_device.h"   // launch_kernel, allow_max_lds, kMaxDynLds; <hip/hip_runtime.h> and include/avae.h with it

namespace avae {

// Rows cut into at most max_slices slices, each a whole number of tiles and never shorter than min_rows (the last one apart):
// slice i covers rows [i * slice_rows, min(rows, (i + 1) * slice_rows)), none is empty, n_slices is 0 only for rows <= 0.  A
// function of rows alone: the determinism contract of every plan built from it.
struct RowSlices { int slice_rows, n_slices; };
inline RowSlices row_slices(long long rows, int max_slices, int min_rows, int tile) {
    if (rows <= 0) return {min_rows, 0};
    const long long per = (rows + max_slices - 1) / max_slices;
    const int slice_rows = (int)std::max<long long>(min_rows, (per + tile - 1) / tile * tile);
    return {slice_rows, (int)((rows + slice_rows - 1) / slice_rows)};
}

// tiles >= 1 tiles cut into about `want` >= 1 splits of at least min_per tiles: split s covers the tiles
// [s * tiles_per_split, min(tiles, (s + 1) * tiles_per_split)), none is empty.
struct TileSplits { int tiles_per_split, n_splits; };
inline TileSplits tile_splits(long long tiles, long long want, long long min_per) {
    const long long per = std::max<long long>(min_per, (tiles + want - 1) / want);
    return {(int)per, (int)((tiles + per - 1) / per)};
}

// No Inf, no NaN: the exponent bits are not all ones.
__device__ __forceinline__ bool latent_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// One latent dimension of one (query, gallery row) pair, added to the running sum.  THE definition of the distance: every
// distance the library returns or embeds (avae_latent_topk, avae_embed_*) comes out of a chain of these over j = 0 .. n_z - 1
// starting from +0.0f, then latent_dist_finish.  Symmetric in its two rows bit for bit (d enters squared, t as a product of both
// sides, iv as a sum).
// Every float operation is the one written: the value of a pair must not depend on which file, instantiation, tile or lane formed
// it.  The .hip files say `#pragma clang fp contract(off)` at their namespace scope, which a function in a header is outside of, so
// each body carries the pragma itself: it ends with the body, and nothing has to be put back for the code after it.
template <int METRIC>
__device__ __forceinline__ float latent_dist_step(float acc, float mq, float vq, float iq, float mg, float vg, float ig) {
#pragma clang fp contract(off)
    const float d = mq - mg;
    if (METRIC == AVAE_METRIC_L2) return __builtin_fmaf(d, d, acc);
    const float t = vq - vg;
    acc = __builtin_fmaf(t * iq, t * ig, acc);
    return __builtin_fmaf(d * d, iq + ig, acc);
}
template <int METRIC> __device__ __forceinline__ float latent_dist_finish(float acc) {
#pragma clang fp contract(off)
    return METRIC == AVAE_METRIC_L2 ? acc : 0.5f * acc;
}

}  // namespace avae
