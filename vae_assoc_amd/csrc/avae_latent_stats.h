// Per-dimension posterior diagnostics (avae_latent_stats; include/avae.h): the plan, the scratch layout and
// the kernel arguments shared by the host (avae_host.hip) and the kernels (avae_latent_stats.hip).
//
// Two launches:
//   k_latent_stats        grid (row slices, work items).  The work items are one per modality m (the column sums of modality m over
//                         the rows that have it, and the n_z x n_z Gram of its shifted means) and one per pair s < d (the column
//                         sums of both sides over the rows that have both).  A workgroup streams its slice once, in row order, and
//                         writes ONE partial per (slice, item) to the scratch: a row count, the shift, and fp64 sums of the SHIFTED
//                         values.  The shift of a column is its value in the first row of the item's row set inside the slice, so
//                         the sums hold deviations of the size of the spread, whatever the mean is.
//   k_latent_stats_merge  one thread per output entry: the slices' partials -> (count, mean, M2, co-moment) each, combined in slice
//                         order by Chan's formula in fp64, then divided by the count; NaN for an empty set.
// No atomics, one fixed order of every sum: the result is a pure function of the input bits, rows, n_z and the flags.  The row
// partition is a function of rows alone and an item reads only its own modalities and flag columns, so a call on a subset of the
// modalities gives the bits of the full call.
#pragma once
#include "avae_latent_common.h"

namespace avae {

constexpr int kStatsThreads = 256;
constexpr int kStatsMaxNz = 64;             // avae_config.n_z's bound
constexpr int kStatsChunk = 64;             // rows of one LDS tile of the Gram
constexpr int kStatsLd = kStatsMaxNz + 4;   // floats per LDS tile row: 16-byte aligned rows, the pad spreads the rows over the banks
constexpr int kStatsMinSliceRows = 256;     // a slice is a whole number of LDS tiles and never shorter than this (the last one apart)
constexpr int kStatsMaxSlices = 256;        // bounds the scratch and the merge; one heavy workgroup per CU at large row counts
constexpr int kStatsMaxSums = 7;            // fp64 sums a thread hands to the workgroup's reduction, at most (the pair item)

struct StatsPlan {
    int row_tile = kStatsMinSliceRows;      // rows per slice: slice i covers rows [i * row_tile, min(rows, (i + 1) * row_tile))
    int n_slices = 0;                       // 0 only for rows == 0; no slice is empty
};

// The row partition: a function of rows alone.
inline StatsPlan stats_plan(long long rows) {
    const RowSlices r = row_slices(rows, kStatsMaxSlices, kStatsMinSliceRows, kStatsChunk);
    return StatsPlan{r.slice_rows, r.n_slices};
}

// Scratch layout, in doubles.  Modality partial (slice, m) at ((slice * M + m) * mod_stride):
//   n | shift [nz] | sum d [nz] | sum d*d [nz] | sum exp(lv) [nz] | sum kl [nz] | Gram sum d_i*d_j [nz][nz]
// Pair partial (slice, p), p the index of s < d in lexicographic order, behind all modality partials at ((slice * P + p) * pair_stride):
//   n | shift_s [nz] | shift_d [nz] | sum d_s | sum d_d | sum d_s*d_s | sum d_d*d_d | sum d_s*d_d | sum assoc    ([nz] each)
// A partial whose n is 0 holds nothing else.
__host__ __device__ inline size_t stats_mod_stride(int nz) { return 1 + 5 * (size_t)nz + (size_t)nz * nz; }
__host__ __device__ inline size_t stats_pair_stride(int nz) { return 1 + 8 * (size_t)nz; }
__host__ __device__ inline int stats_pairs(int n_mod) { return n_mod * (n_mod - 1) / 2; }
__host__ __device__ inline int stats_pair_index(int n_mod, int s, int d) { return s * n_mod - s * (s + 1) / 2 + (d - s - 1); }   // s < d
inline size_t stats_scratch_bytes(int n_slices, int n_mod, int nz) {
    return (size_t)n_slices * (n_mod * stats_mod_stride(nz) + stats_pairs(n_mod) * stats_pair_stride(nz)) * sizeof(double);
}
// What a call can ask for at most (256 slices, 4 modalities, n_z = 64): 42,487,808 bytes.  The handle allocates this much once.
constexpr size_t kStatsScratchBytes =
    (size_t)kStatsMaxSlices * (AVAE_MAX_MODALITIES * (1 + 5 * kStatsMaxNz + kStatsMaxNz * kStatsMaxNz) +
                               (AVAE_MAX_MODALITIES * (AVAE_MAX_MODALITIES - 1) / 2) * (1 + 8 * kStatsMaxNz)) * sizeof(double);

struct StatsArgs {
    const float* mu[AVAE_MAX_MODALITIES];    // dense [rows][nz]; NULL: the modality is absent from every row
    const float* lv[AVAE_MAX_MODALITIES];
    const uint8_t* present;                  // [rows][n_mod], or NULL: every given modality on every row
    double* scratch;
    long long rows;
    int n_mod, nz, n_slices, row_tile;
    int want_cov;                            // 0: out.cov is NULL and the Gram is skipped
    avae_latent_stats_out out;
};

void launch_latent_stats(const StatsArgs& a, hipStream_t s);
void launch_latent_stats_merge(const StatsArgs& a, hipStream_t s);

}  // namespace avae
