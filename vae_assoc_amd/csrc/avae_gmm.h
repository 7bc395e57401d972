// Mixture prior fitted to the posteriors (avae_gmm_fit / avae_gmm_score; include/avae.h): the plan, the
// scratch layout and the kernel arguments shared by the host (avae_host.hip) and the kernels (avae_gmm.hip).
//
// Two launches per EM iteration, the whole loop enqueued on the caller's stream with no host synchronisation inside:
//   k_gmm_estep  grid = row slices.  A workgroup of 4 wave64s keeps the K components in LDS -- (m, -1/2 exp(-s)) pairs and the
//                per-component constant log pi_k - 1/2 sum_j (s_kj + log 2pi) -- and streams its slice in tiles of 64 rows (mu, and
//                v = expf(lv) formed while staging; the next tile is on its way from memory meanwhile).  Phase 1, lane = row, wave w =
//                the components [4w, 4w + 4), [4w + 16, 4w + 20), ...: the exponents as fp32 fused multiply-add chains over j in
//                index order, the row's max, p = expf(E - max), their sum in k order (in fp64, rounded once), ll = max + logf(sum),
//                r = p / sum into an LDS tile [64][K + 1].  Phase 2, thread = column j and the components g, g + G, ...: the tile's rows in order, r (mu - m)
//                and r ((mu - m)^2 + v) as fp64 fused multiply-adds (mu - m formed in fp64: the products are exact) into
//                registers that live for the whole slice; R_k likewise.  ll is added in fp64 per row position of the tiles (lane = row), the 64 positions in order at the end.
//                A row with a non-finite entry is selected away (zeros staged, r = 0).  ONE partial per slice goes to the scratch.
//   k_gmm_mstep  one thread per (k, j), in blocks of 256: the slices' partials combined in slice order in fp64, the update, the
//                next fp32 parameters and bound[t].  After the last E-step one block only writes bound[n_iters] and n_used.
// avae_gmm_score is k_gmm_estep with the per-row outputs switched on and the sums switched off.
// No atomics, one fixed order of every sum.  The row partition is a function of rows alone.
#pragma once
#include "avae_latent_common.h"

namespace avae {

constexpr int kGmmThreads = 256;
constexpr int kGmmWaves = kGmmThreads / 64;
constexpr int kGmmTile = 64;                // rows of one LDS tile; lane = row in phase 1
constexpr int kGmmTileLd = kGmmTile + 1;    // [n_z][rows + pad]: the pad spreads the staging stores and phase 2's reads over the banks
constexpr int kGmmMaxNz = 64;               // avae_config.n_z's bound
constexpr int kGmmMaxK = 64;
constexpr int kGmmMinSliceRows = kGmmTile;  // a slice is a whole number of tiles (the last one apart): small inputs spread over the CUs
constexpr int kGmmMaxSlices = 256;          // bounds the scratch and the merge; one workgroup per CU at large row counts
constexpr int kGmmOwn = kGmmMaxK / kGmmWaves;   // components of one wave (phase 1) / of one thread (phase 2), at most
static_assert(kGmmMinSliceRows % kGmmTile == 0, "a slice is a whole number of tiles");

struct GmmPlan {
    int slice_rows = kGmmMinSliceRows;      // slice i covers rows [i * slice_rows, min(rows, (i + 1) * slice_rows))
    int n_slices = 0;                       // 0 only for rows == 0; no slice is empty
};

// The row partition: a function of rows alone.
inline GmmPlan gmm_plan(long long rows) {
    const RowSlices r = row_slices(rows, kGmmMaxSlices, kGmmMinSliceRows, kGmmTile);
    return GmmPlan{r.slice_rows, r.n_slices};
}

// Scratch, in doubles.  The partial of a slice at slice * gmm_part_stride(K, nz):
//   sum ll | used rows | R [K] | S1 [K][nz] | S2 [K][nz]
// Behind the partials of all slices: two parameter sets of gmm_param_floats(K, nz) fp32 each, weights [K] | means [K][nz] |
// logvars [K][nz], which the iterations between the first and the last alternate between.
__host__ __device__ inline size_t gmm_part_stride(int K, int nz) { return 2 + (size_t)K + 2 * (size_t)K * nz; }
__host__ __device__ inline size_t gmm_param_floats(int K, int nz) { return (size_t)K + 2 * (size_t)K * nz; }
inline size_t gmm_scratch_bytes(int n_slices, int K, int nz) {
    return (size_t)n_slices * gmm_part_stride(K, nz) * sizeof(double) + 2 * gmm_param_floats(K, nz) * sizeof(float);
}
// What a call can ask for at most (256 slices, K = 64, n_z = 64): 16,978,432 bytes.  The handle allocates this much once.
constexpr size_t kGmmScratchBytes =
    (size_t)kGmmMaxSlices * (2 + kGmmMaxK + 2 * kGmmMaxK * kGmmMaxNz) * sizeof(double) +
    2 * (size_t)(kGmmMaxK + 2 * kGmmMaxK * kGmmMaxNz) * sizeof(float);

// Dynamic LDS of k_gmm_estep, in the kernel's order: (m, -1/2 exp(-s)) [K][nz] float2 | mu tile [nz][65] | v tile [nz][65] |
// r tile [64][K + 1] | constants [K] | non-finite flags [64].  K = 64, n_z = 64: 32,768 + 2 * 16,640 + 16,640 + 256 + 256
// = 83,200 bytes of the CU's 160 KiB.
__host__ __device__ inline size_t gmm_lds_bytes(int K, int nz) {
    return ((size_t)2 * K * nz + (size_t)2 * nz * kGmmTileLd + (size_t)kGmmTile * (K + 1) + (size_t)K + kGmmTile) * sizeof(float);
}
static_assert(((size_t)2 * kGmmMaxK * kGmmMaxNz + (size_t)2 * kGmmMaxNz * kGmmTileLd + (size_t)kGmmTile * (kGmmMaxK + 1) +
               (size_t)kGmmMaxK + kGmmTile) * sizeof(float) <= 100 * 1024,
              "K = 64, n_z = 64 has to fit well inside the LDS of one CU");

struct GmmArgs {
    const float* mu; const float* lv;        // dense [rows][nz]; lv NULL: points (v = 0)
    const float* w_in; const float* m_in; const float* s_in;     // the parameters this E-step scores: [K], [K][nz], [K][nz]
    float* w_out; float* m_out; float* s_out;                    // what the M-step writes (may be the *_in arrays themselves)
    double* part;                            // [n_slices][gmm_part_stride]
    double* bound;                           // the M-step writes bound[0]
    int32_t* n_used;                         // written by the final merge
    float* ll; int32_t* component; float* resp;                  // per-row outputs (avae_gmm_score), nullable
    long long rows;
    int nz, K, n_slices, slice_rows;
    int want_stats;                          // 0: no partial is written (avae_gmm_score)
    int final_pass;                          // M-step: 1 = only bound[0] and n_used, one block
    float var_floor;
};

void launch_gmm_estep(const GmmArgs& a, hipStream_t s);
void launch_gmm_mstep(const GmmArgs& a, hipStream_t s);

}  // namespace avae
