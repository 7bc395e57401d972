// Cross-modal retrieval (avae_latent_topk; include/avae.h): the plan and the kernel arguments shared by the
// host (avae_host.hip) and the kernels (avae_retrieve.hip).
//
// Two launches per chunk of at most kTopkChunkRows queries:
//   k_latent_topk        grid (query tiles, gallery splits).  A workgroup of 8 wave64s keeps its 64 queries' (mu, v, iv) in LDS,
//                        streams its slice of the gallery through LDS in tiles of 64 rows (v = expf(lv), iv = expf(-lv) formed
//                        while staging), every thread holds a 4 x 2 block of distances in registers, and a sorted list of the k
//                        best (key, index) per query lives in LDS.  The list of (query, split) goes to the scratch.
//   k_latent_topk_merge  one wave64 per query: a k-step merge of the splits' sorted lists.
// A list entry is ONE 64-bit word, (order key of the distance) << 32 | gallery index, so that unsigned comparison IS the total
// order (isnan(dist), dist, index): the key of a float is its bits with the sign handled the usual way (distances are sums of
// non-negative addends, so in fact always their own bits with the top bit set), every NaN has the key of the canonical quiet NaN,
// and an empty slot is all ones (it sorts last and comes out as index -1, distance +Inf).
#pragma once
#include "avae_latent_common.h"

namespace avae {

constexpr int kTopkThreads = 512;
constexpr int kTopkQueryTile = 64;       // 16 x 32 threads, 4 queries x 2 gallery rows each
constexpr int kTopkGalleryTile = 64;
constexpr int kTopkQueryLd = kTopkQueryTile + 4;      // LDS images are [n_z][rows + pad]: the pads spread the staging stores over
constexpr int kTopkGalleryLd = kTopkGalleryTile + 2;  // the banks and keep the 16- / 8-byte row reads aligned
constexpr int kTopkStashLd = 9;          // the selection path's [64 candidates][8 queries + 1] distances of one wave
constexpr int kTopkMaxNz = 64;           // avae_config.n_z's bound (the staging registers hold a gallery tile of 64 x 64 x 2 floats)
constexpr int kTopkChunkRows = 16384;    // queries per pair of launches
constexpr int kTopkTargetGroups = 1024;  // workgroups a launch should have: four rounds of one per CU (n_z = 64: one fits)
constexpr int kTopkMaxSplits = 256;      // the merge keeps at most 4 list heads per lane
constexpr int kTopkMinTilesPerSplit = 4; // a split pays k insertions before its filter bites
constexpr unsigned long long kTopkEmpty = ~0ull;

struct TopkPlan {
    int query_tile = kTopkQueryTile, gallery_tile = kTopkGalleryTile;
    int chunk_rows = 0;         // queries per pair of launches = min(rows, kTopkChunkRows)
    int n_splits = 0;           // gallery slices; 0: an empty gallery (the merge launch alone fills the outputs)
    int tiles_per_split = 0;    // split s covers gallery tiles [s * tiles_per_split, min(tiles, (s + 1) * tiles_per_split)): none is empty
    size_t scratch_bytes = 0;   // chunk_rows * n_splits * k lists entries of 8 bytes
};

// The shapes of the two launches: a function of (rows, gallery_rows, k) alone.  The gallery is cut so that the launch has about
// kTopkTargetGroups workgroups however few queries there are; queries are worked in chunks so that the scratch stays below
// kTopkScratchBytes however many there are.
inline TopkPlan topk_plan(long long rows, long long gallery_rows, int k) {
    TopkPlan p;
    p.chunk_rows = (int)std::min<long long>(rows, kTopkChunkRows);
    if (rows <= 0 || gallery_rows <= 0) return p;
    const long long q_tiles = (p.chunk_rows + kTopkQueryTile - 1) / kTopkQueryTile;
    const long long g_tiles = (gallery_rows + kTopkGalleryTile - 1) / kTopkGalleryTile;
    long long want = (kTopkTargetGroups + q_tiles - 1) / q_tiles;
    want = std::max<long long>(1, std::min<long long>(want, kTopkMaxSplits));
    const TileSplits t = tile_splits(g_tiles, want, kTopkMinTilesPerSplit);
    p.tiles_per_split = t.tiles_per_split; p.n_splits = t.n_splits;
    p.scratch_bytes = (size_t)p.chunk_rows * p.n_splits * k * sizeof(unsigned long long);
    return p;
}
// What topk_plan can ask for at most (k = 64): chunk_rows * n_splits <= 64 * (kTopkTargetGroups + 256 query tiles).  The handle
// allocates this much once.
constexpr size_t kTopkScratchBytes = (size_t)kTopkQueryTile * (kTopkTargetGroups + kTopkChunkRows / kTopkQueryTile) * 64 * 8;

// Dynamic LDS of k_latent_topk, in the kernel's order: lists [k][64] | filters [64] | stashes | query images | gallery images (an
// image = [n_z][rows + pad] floats; three per side -- mu, v, iv -- under SYMKL, mu alone under L2).  n_z = 64, k = 64, SYMKL:
// 154,368 bytes of the CU's 160 KiB.
inline size_t topk_lds_bytes(int nz, int k, int metric) {
    const size_t images = metric == AVAE_METRIC_L2 ? 1 : 3;
    return (size_t)k * kTopkQueryTile * sizeof(unsigned long long) +
           (kTopkQueryTile + (size_t)(kTopkThreads / 64) * kTopkGalleryTile * kTopkStashLd +
            images * nz * (kTopkQueryLd + kTopkGalleryLd)) * sizeof(float);
}

struct TopkArgs {
    const float* q_mu; const float* q_lv;     // the chunk's queries, dense [rows][nz] (lv NULL under L2)
    const float* g_mu; const float* g_lv;     // the gallery, dense [gallery_rows][nz]
    unsigned long long* part;                 // [rows][n_splits][k] sorted lists
    int* index; float* dist;                  // nullable outputs of the chunk, dense [rows][k]
    int rows, gallery_rows, nz, k;
    int n_splits, tiles_per_split;
    int metric;
};

void launch_latent_topk(const TopkArgs& a, hipStream_t s);
void launch_latent_topk_merge(const TopkArgs& a, hipStream_t s);

}  // namespace avae
