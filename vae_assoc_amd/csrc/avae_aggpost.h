// Aggregate-posterior log-density (avae_agg_logpdf; include/avae.h): the plan, the scratch layout and the
// kernel arguments shared by the host (avae_host.hip) and the kernels (avae_aggpost.hip).
//
// Two launches per chunk of at most kAggChunkRows queries:
//   k_agg_logpdf        grid (query tiles, gallery slices).  A workgroup of 8 wave64s keeps its 64 queries' z in LDS and streams
//                       its slice of the gallery through LDS in tiles of 64 rows (mu, -0.5 * expf(-lv) and -0.5 * lv formed while
//                       staging).  Lane = query everywhere, so a gallery value is one broadcast LDS read for the whole wave.
//                       Marginals: wave w owns the columns w, w + 8, ... and walks the tile's rows in order in blocks of 8 -- 8
//                       exponents, their max against the running max, ONE rescale, 8 exponentials: two state registers per
//                       (query, column).  Joint: wave r owns rows [8r, 8r + 8) of every tile: the 8 exponents are sums over
//                       j = 0 .. n_z-1 in index order, then the same block update of the (query, r) state; the 8 states of a query
//                       are combined in r order when the slice is done.  One (max, scaled sum) fp32 pair per (query, slice,
//                       column) goes to the scratch, the joint in column 0.
//   k_agg_logpdf_merge  one wave64 per query: the slices' pairs combined in slice order in fp64, log G' and the constant
//                       subtracted in fp64, one rounding to fp32.  It alone writes the answer of an empty gallery.
// No atomics.  The gallery partition is a function of gallery_rows alone and every block of 8 is the gallery rows [8b, 8b + 8), so
// the value of a query is a pure function of its own bits, its exclude entry and the gallery.
#pragma once
#include "avae_latent_common.h"

namespace avae {

constexpr int kAggThreads = 512;
constexpr int kAggQueryTile = 64;        // lane = query
constexpr int kAggGalleryTile = 64;
constexpr int kAggBlock = 8;             // gallery rows per running-max update
constexpr int kAggWaves = kAggThreads / 64;
constexpr int kAggQueryLd = kAggQueryTile + 1;      // [n_z][rows + pad]: the pad spreads the staging stores over the banks
constexpr int kAggGalleryLd = kAggGalleryTile + 4;  // ... and keeps the 16-byte reads of four rows aligned
constexpr int kAggMaxNz = 64;            // avae_config.n_z's bound
constexpr int kAggChunkRows = 2048;      // queries per pair of launches
constexpr int kAggMaxSlices = 64;
constexpr int kAggMinSliceRows = 1024;   // 16 tiles: a slice pays its set-up and one scratch row per query
static_assert(kAggGalleryTile == kAggWaves * kAggBlock, "the joint pass gives wave r the block r of every tile");
static_assert(kAggMinSliceRows % kAggGalleryTile == 0, "a slice is a whole number of tiles");

struct AggPlan {
    int query_tile = kAggQueryTile;
    int chunk_rows = 0;          // queries per pair of launches = min(rows, kAggChunkRows)
    int slice_rows = kAggMinSliceRows;   // slice i covers the gallery rows [i * slice_rows, min(gallery_rows, (i + 1) * slice_rows))
    int n_slices = 0;            // 0 only for an empty gallery; no slice is empty
};

// The gallery partition is a function of gallery_rows ALONE (the determinism contract); rows only sets the chunk.
inline AggPlan agg_plan(long long rows, long long gallery_rows) {
    AggPlan p;
    p.chunk_rows = (int)std::min<long long>(std::max<long long>(rows, 0), kAggChunkRows);
    const RowSlices r = row_slices(gallery_rows, kAggMaxSlices, kAggMinSliceRows, kAggGalleryTile);
    p.slice_rows = r.slice_rows; p.n_slices = r.n_slices;
    return p;
}
// Scratch: part[query of the chunk][slice][1 + n_z] pairs (running max, sum scaled by it) of fp32; column 0 is the joint.
inline size_t agg_scratch_bytes(const AggPlan& p, int nz) {
    return (size_t)p.chunk_rows * p.n_slices * (1 + (size_t)nz) * 2 * sizeof(float);
}
// What a call can ask for at most (2048 queries, 64 slices, n_z = 64): 68,157,440 bytes.  The handle allocates this much once.
constexpr size_t kAggScratchBytes = (size_t)kAggChunkRows * kAggMaxSlices * (1 + kAggMaxNz) * 2 * sizeof(float);

// Dynamic LDS of k_agg_logpdf, in the kernel's order: gallery images mu, -iv/2, -lv/2 [n_z][68] each | the joint's [8][64] pairs |
// z image [n_z][65].  n_z = 64: 52,224 + 4,096 + 16,640 = 72,960 bytes of the CU's 160 KiB (two workgroups per CU).
inline size_t agg_lds_bytes(int nz) {
    return ((size_t)nz * (kAggQueryLd + 3 * kAggGalleryLd) + (size_t)kAggWaves * kAggQueryTile * 2) * sizeof(float);
}
static_assert(((size_t)kAggMaxNz * (kAggQueryLd + 3 * kAggGalleryLd) + (size_t)kAggWaves * kAggQueryTile * 2) * sizeof(float) <= kMaxDynLds,
              "n_z = 64 has to fit the LDS of one CU");

struct AggArgs {
    const float* z;                 // the chunk's queries, dense [rows][nz]
    const float* g_mu; const float* g_lv;     // the gallery, dense [gallery_rows][nz]
    const int32_t* exclude;         // the chunk's [rows], or NULL
    float2* part;                   // [rows][n_slices][1 + nz]
    float* joint; float* marginal;  // nullable outputs of the chunk, dense [rows] / [rows][nz]
    int rows, gallery_rows, nz;
    int n_slices, slice_rows;
};

void launch_agg_logpdf(const AggArgs& a, hipStream_t s);
void launch_agg_logpdf_merge(const AggArgs& a, hipStream_t s);

}  // namespace avae
