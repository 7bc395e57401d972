// Black-box search around a cost (avae_search_sample / avae_search_update; include/avae.h): the launch shapes,
// the kernel arguments shared by the host (avae_host.hip) and the kernels (avae_search.hip), and every operation in its order.
//
// k_search_sample  rows (p, r) of x [P][R][n] are dealt in tiles of search_tile_rows(n) consecutive rows, one workgroup of 256
//                  threads per tile (so a workgroup writes one dense range of x).  nq = ceil(n / 4) quads per row.
//   1. thread i takes the (row, quad) items i, i + 256, ... of the tile: one Philox4x32-10 block, counter (problem_offset + p, r,
//      quad, iteration), key (seed lo, seed hi ^ 'srch'), the four normals of box_muller4 (avae_philox.h), and for the dimensions
//      d = 4 quad + e < n:  y = fma(sqrtf(var[p][d]), normal_e, mean[p][d])  (IEEE square root).  Without a map y is stored.
//   2. with a map (G groups of g consecutive dimensions) the tile's y wait in LDS and thread i takes the elements i, i + 256, ...
//      of the tile: dimension d = group * g + j gives  acc = b[p][d];  for k = 0 .. g - 1: acc = fma(A[group][j][k], y[group * g + k],
//      acc);  x = acc.
//   LDS 4 KiB (the tile's y), 54 VGPRs, no scratch.
// k_search_update  one workgroup of 256 threads per problem.  All arithmetic below is IEEE double, no contraction, rounded once
//   where a float leaves.  "Thread order": thread i adds its rollouts r = i, i + 256, i + 512, i + 768 (those that count) in that
//   order from 0; THE TREE: the 256 partial values combine as  for s = 128, 64 .. 1: v[i] = v[i] (op) v[i + s], i < s.
//   1. c_r = (double) cost[p][r]; a rollout counts when c_r is finite.  F = their number, cmin / cmax their exact minimum / maximum,
//      the best rollout the one with the lowest c_r, the lower r on a tie (all four through one tree).
//      If F > 0 and cmin < best_cost[p] (a comparison of floats): best_cost[p] = cmin, best_x[p] = x[p][best rollout].
//   2. if F == 0 or frozen[p] != 0: avg_cost = min_cost = moved = NaN, nothing else is written.  Else:
//   3. S = sum c_r (thread order, THE TREE), cbar = S / F;  Q = sum (c_r - cbar)^2 (the same order), sd = sqrt(Q / F).
//   4. weights.  If sd <= 1e-8 |cbar|: w_r = 1.  Else
//        PI-BB : w_r = exp(-h * (c_r - cmin) / ((cmax - cmin) + 1e-6))         (h = eliteness)
//        CEM   : rank_r = #{j counting: c_j < c_r, or c_j == c_r and j < r};  w_r = rank_r < mu ? 1 / mu : 0    (mu = eliteness)
//        CMA-ES: w_r = rank_r < mu ? log(mu + 0.5) - log(rank_r + 1) : 0
//      a rollout that does not count has w_r = 0.  W = sum w_r (thread order, THE TREE);  w_r = w_r / W.
//   5. thread i owns the dimensions d = i, i + 256, ...  With m0 = (double) mean[p][d], v0 = (double) var[p][d]:
//        m1 = sum_r w_r * (double) x[p][r][d]              r ascending from 0, a product and a sum each, rollouts with w_r == 0 skipped
//        c  = cov_update == CEM ? m1 : m0
//        s  = sum_r w_r * ((x - c) * (x - c))              the same order and skipping
//        v1 = (1 - lr) * v0 + lr * s
//   6. bounds, each only where its option is >= 0: v1 = min(v1, abs_upper) by comparison (v1 > abs_upper ? abs_upper : v1);  vmax =
//      the maximum of v1 over d (a thread's own in ascending d, then THE TREE, by comparison y > x ? y : x);  lower = abs_lower (or
//      none), and with rel_lower >= 0: lower = max(lower, rel_lower * vmax) (the product alone where there is no abs_lower);
//      v1 = v1 < lower ? lower : v1.
//   7. moved = sqrt(sum_d (m1 - m0)^2)  (a thread's own dimensions ascending from 0, THE TREE).
//   8. mean[p][d] = (float) m1, var[p][d] = (float) v1, n_applied[p] += 1, avg_cost = (float) cbar, min_cost = (float) cmin,
//      moved_out = (float) moved;  frozen[p] = 1 if moved < tol.
//   LDS 18 KiB (the weights as doubles, the counting costs, the tree's columns), 65 VGPRs, no scratch.
// Neither kernel uses atomics or scratch memory or reads or writes anything of the handle.
#pragma once
#include "avae_latent_common.h"

namespace avae {

constexpr int kSearchThreads = 256;
constexpr int kSearchMaxN = 1024, kSearchMaxR = 1024, kSearchMaxG = 64;
constexpr int kSearchDims = kSearchMaxN / kSearchThreads;        // dimensions (and rollouts) a thread owns, at most
constexpr int kSearchTileFloats = 1024;                          // LDS floats of a sample tile
constexpr unsigned kSearchSalt = 0x73726368u;                    // 'srch'

__host__ __device__ inline int search_quads(int n) { return (n + 3) / 4; }
// rows of a sample tile: as many as fit kSearchTileFloats floats at 4 * quads floats a row
__host__ __device__ inline int search_tile_rows(int n) { return kSearchTileFloats / (4 * search_quads(n)); }

struct SearchSampleArgs {
    const float* mean;            // [P][n]
    const float* var;             // [P][n]
    const float* proj_A;          // [G][g][g] or NULL
    const float* proj_b;          // [P][n] or NULL
    float* x;                     // [P][R][n]
    long long rows;               // P * R
    unsigned long long seed;
    unsigned problem0, iteration;
    int R, n, G, g;
};

struct SearchUpdateArgs {
    const float* x;               // [P][R][n]
    const float* cost;            // [P][R]
    float* mean;                  // [P][n]
    float* var;                   // [P][n]
    int32_t* n_applied;           // [P]
    int32_t* frozen;              // [P]
    float* best_cost;             // [P]
    float* best_x;                // [P][n]
    float* avg_cost;              // [P] or NULL
    float* min_cost;              // [P] or NULL
    float* moved;                 // [P] or NULL
    int R, n;
    int weighting, cov_update, mu;
    double h, lr, rel_lower, abs_lower, abs_upper, tol;
};

void launch_search_sample(const SearchSampleArgs& a, hipStream_t s);
void launch_search_update(const SearchUpdateArgs& a, int P, hipStream_t s);

}  // namespace avae
