// 2-D t-SNE map of the posteriors (avae_embed_calibrate / avae_embed_iterate; include/avae.h): the plan, the
// scratch layout and the kernel arguments shared by the host (avae_host.hip) and the kernels (avae_embed.hip).
//
// The N x N affinities never exist in memory: p_ij is recomputed in every iteration from the pair's distance (n_z to 3 n_z fused
// multiply-adds on operands in LDS) and three numbers per row (beta, shift, norm).  Launches, all enqueued on the caller's stream
// with no host synchronisation inside:
//   k_embed_scan       one thread per row: the row's "used" byte (no non-finite entry) and one count per block of 256 rows
//   k_embed_calibrate  a workgroup of 4 wave64s owns 64 rows, keeps their (mu, v, iv) in LDS and streams ALL rows through LDS in
//                      tiles of 64, once for the minimum and once per try of the search; every thread holds a 4 x 4 block of pairs;
//                      the rows' sums are fp32 inside a tile, fp64 across the tiles (per thread, tiles in order) and across the
//                      16 threads of a row (a fixed shuffle tree); finished rows freeze, the loop ends when all 64 are finished
//   k_embed_forces     grid (row tiles, splits of the streamed side): the same tiles, plus (beta, shift, c, y) per row of either
//                      side; per pair p_ij, w_ij and the six sums A (2), R (2), sum w, sum p (log p - log w) (the p log p part only
//                      in the first pass of a call: it does not depend on Y); ONE partial per (row, split) to the scratch
//   k_embed_update     blocks of 256 rows: every block adds all rows' sum w and KL parts for itself in a fixed order (Z, KL), then
//                      one thread per row merges the splits in split order in fp64, forms the gradient and applies the update
//   k_embed_center     subtracts the mean the last k_embed_update left in the scratch
// No atomics, one fixed order of every sum.  The split plan is a function of rows alone.
#pragma once
#include "avae_latent_common.h"

namespace avae {

constexpr int kEmbedThreads = 256;
constexpr int kEmbedTile = 64;               // rows of either side of a tile: 16 x 16 threads, 4 x 4 pairs each
constexpr int kEmbedLd = kEmbedTile + 4;     // LDS images are [n_z][rows + pad]: the pad spreads the staging stores over the banks
                                             // and keeps the 16-byte row reads aligned
constexpr int kEmbedMaxNz = 64;              // avae_config.n_z's bound
constexpr int kEmbedMaxRows = 65536;         // calibration is O(rows^2 x tries)
constexpr int kEmbedTargetGroups = 1024;     // workgroups k_embed_forces should have: four rounds of one per CU
constexpr int kEmbedParts = 6;               // A0 | A1 | R0 | R1 | sum w | sum p (log p - log w) (or - sum p log w alone)
constexpr int kEmbedScanRows = 256;          // rows per block of k_embed_scan and k_embed_update
constexpr float kEmbedBetaMax = 1.2676506002282294e30f, kEmbedBetaMin = 7.8886090522101181e-31f;   // 2^100, 2^-100: the search's beta stays inside

struct EmbedPlan {
    int row_tile = kEmbedTile;
    int n_splits = 0;           // slices of the streamed side; 0 only for rows == 0
    int tiles_per_split = 0;    // split s covers the tiles [s * tiles_per_split, min(tiles, (s + 1) * tiles_per_split)): none is empty
    size_t scratch_bytes = 0;   // what a call with this many rows touches
};

// Scratch: used bytes [kEmbedMaxRows] | block counts int32 [256] | mean double [2] | pad | partials double [kEmbedParts][slots] |
// p log p parts double [slots], slot = row * n_splits + split.
constexpr size_t kEmbedMaxSlots = 2 * (size_t)kEmbedMaxRows;   // rows * n_splits <= 64 * tiles * n_splits, and tiles * n_splits <= 2048 (1023 tiles in 2 splits)
constexpr size_t kEmbedOffCount = kEmbedMaxRows;
constexpr size_t kEmbedOffMean = kEmbedOffCount + (kEmbedMaxRows / kEmbedScanRows) * sizeof(int32_t);
constexpr size_t kEmbedOffPart = kEmbedOffMean + 128;
static_assert(kEmbedOffPart % 128 == 0, "the partials start on a line");
constexpr size_t kEmbedScratchBytes = kEmbedOffPart + (kEmbedParts + 1) * kEmbedMaxSlots * sizeof(double);

// The shapes of k_embed_forces: a function of rows alone.  The streamed side is cut so that the launch has about
// kEmbedTargetGroups workgroups however few rows there are.
inline EmbedPlan embed_plan(long long rows) {
    EmbedPlan p;
    if (rows <= 0) return p;
    const long long tiles = (rows + kEmbedTile - 1) / kEmbedTile;
    const long long want = std::max<long long>(1, std::min<long long>(tiles, (kEmbedTargetGroups + tiles - 1) / tiles));
    const TileSplits t = tile_splits(tiles, want, 1);
    p.tiles_per_split = t.tiles_per_split; p.n_splits = t.n_splits;
    p.scratch_bytes = kEmbedOffPart + (kEmbedParts + 1) * (size_t)rows * p.n_splits * sizeof(double);
    return p;
}

// Dynamic LDS of k_embed_calibrate and k_embed_forces, in the kernels' order: row-side images | streamed-side images (an image =
// [n_z][68] floats; three per side -- mu, v, iv -- under SYMKL, mu alone under L2) | per-row scalars of both sides, 8 x [64] words
// each.  n_z = 64, SYMKL: 2 * 52,224 + 4,096 = 108,544 bytes of the CU's 160 KiB.
constexpr int kEmbedRowWords = 8;            // beta | shift | c | y0 | y1 | used | (calibrate: lo | hi)
__host__ __device__ inline size_t embed_lds_bytes(int nz, int metric) {
    const size_t images = metric == AVAE_METRIC_L2 ? 1 : 3;
    return (2 * images * nz * kEmbedLd + 2 * (size_t)kEmbedRowWords * kEmbedTile) * sizeof(float);
}
static_assert((2 * (size_t)3 * kEmbedMaxNz * kEmbedLd + 2 * (size_t)kEmbedRowWords * kEmbedTile) * sizeof(float) <= kMaxDynLds,
              "n_z = 64 under SYMKL has to fit the LDS of one CU");

struct EmbedArgs {
    const float* mu; const float* lv;        // dense [rows][nz]; lv NULL under L2
    unsigned char* used;                     // scratch: [rows] 1 = the row has no non-finite entry
    int32_t* count;                          // scratch: used rows per block of kEmbedScanRows rows
    double* mean;                            // scratch: [2], written by the evaluating k_embed_update, read by k_embed_center
    double* part;                            // scratch: [kEmbedParts][part_stride]
    double* plogp;                           // scratch: [part_stride]
    size_t part_stride;                      // rows * n_splits
    float* beta; float* shift; float* norm;  // calibration: out of k_embed_calibrate, in of k_embed_forces
    int32_t* tries; int32_t* n_used;         // k_embed_calibrate
    float* y; float* vel; float* gain;       // [rows][2] each
    double* kl;                              // k_embed_update writes kl[0]
    float* grad;                             // nullable [rows][2]
    int rows, nz, metric;
    int n_splits, tiles_per_split;
    int max_tries;
    double log_perp, tol;                    // log(perplexity) and the search's tolerance on the entropy
    int first_pass;                          // k_embed_forces: 1 = also the p log p parts
    int evaluate;                            // k_embed_update: 1 = kl and grad only (the last pass), the state stays
    int center;                              // ... and it leaves the used rows' mean of y in `mean`
    float alpha, mom, lr;
};

void launch_embed_scan(const EmbedArgs& a, hipStream_t s);
void launch_embed_calibrate(const EmbedArgs& a, hipStream_t s);
void launch_embed_forces(const EmbedArgs& a, hipStream_t s);
void launch_embed_update(const EmbedArgs& a, hipStream_t s);
void launch_embed_center(const EmbedArgs& a, hipStream_t s);

}  // namespace avae
