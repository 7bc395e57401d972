// Motion decoding (avae_motion_eval / _fit / _moments; include/avae.h): the launch shapes and the kernel
// arguments shared by the host (avae_host.hip) and the kernels (avae_motion.hip).
//
// A row's P = D * Kb parameters become theta = params * scale + shift (one fma), and a trajectory point is
//   q[t][d] = sum_k phi[t][k] * theta[d][k]  (+ sum_c gain[t][c] * target[d][c]),  then clamped by comparison to [lo_d, hi_d],
// every sum an fp32 fma chain in index order starting from 0.  fp32 VALU work with an inner length of Kb ~ 21: no MFMA.
//
// How a workgroup's 256 threads share the outputs (all three kernels of eval / moments): thread tid < TQ * D owns joint
// d = tid % D and the time points t = s0 + tid / D + j * TQ, j < 4, of the current time slab [s0, s0 + TS); TQ = 256 / D.  So
// consecutive lanes own consecutive (t, d) entries of the dense [T, D] output, and a thread's joint never changes: the sums over
// t of a (row, joint) are a thread's own running value (slabs and j in order) and then a fixed tree over the TQ threads of the
// joint in LDS.  A slab's phi rows (and anchor gains) are staged in LDS, rows padded to an odd length.
//   k_motion_eval     one workgroup per tile of kMotionRows rows; the rows' theta (and the reference parameters' theta) staged once.
//   k_motion_moments  one workgroup per row; per slab the row's S samples stream through two LDS tiles of kMotionRows samples each
//                     (the next tile's 16-byte global loads are in flight while the current one is evaluated), a thread keeps the
//                     running mean and M2 of its <= 4 outputs in registers (the sequential update of avae_impute, sample order).
//   k_motion_fit      one workgroup per tile of kMotionRows rows; thread tid owns parameters tid, tid + 256, ...; time slabs of
//                     kFitSlab points of pinv and of the rows' trajectories staged in LDS, one fma chain over t per parameter.
// No atomics, no scratch, nothing of the handle is read or written.
#pragma once
#include "avae_latent_common.h"

namespace avae {

constexpr int kMotionThreads = 256;
constexpr int kMotionRows = 4;          // rows (eval, fit) or samples (moments) evaluated together: the register block and the LDS tile
constexpr int kMotionJ = 4;             // time points per thread and slab, at most
constexpr int kMotionMaxD = 16, kMotionMaxKb = 64, kMotionMaxT = 1024, kMotionMaxNc = 4;
constexpr int kMotionPhiFloats = 4096;  // LDS floats of a slab's phi rows, at most
constexpr int kMotionMaxSlab = 512;     // time points of a slab, at most (bounds the gain slab)
constexpr int kFitSlab = 64;            // time points of a slab of k_motion_fit
constexpr size_t kMotionMaxLds = 65536;

__host__ __device__ inline int motion_pad(int kb) { return kb | 1; }                       // odd row length: no bank conflicts
__host__ __device__ inline int motion_tq(int D) { return kMotionThreads / D; }
__host__ __device__ inline int motion_slab(int D, int Kb, int T) {
    int ts = kMotionJ * motion_tq(D);
    ts = ts < kMotionPhiFloats / motion_pad(Kb) ? ts : kMotionPhiFloats / motion_pad(Kb);
    ts = ts < kMotionMaxSlab ? ts : kMotionMaxSlab;
    return ts < T ? ts : T;
}

struct MotionArgs {
    const float* params;          // eval: [rows][P]; moments: samples [rows][S][P]
    const float* phi;             // [T][Kb]
    const float* scale;           // [P] or NULL (1)
    const float* shift;           // [P] or NULL (0)
    const float* limits;          // [D][2] or NULL
    const float* gain;            // [T][nc] or NULL
    const float* target;          // [rows][D][nc] or NULL
    const float* ref_traj;        // eval: [rows][T][D] or NULL
    const float* ref_params;      // eval: [rows][P] or NULL
    float* traj;                  // eval: [rows][T][D] or NULL; moments: the mean
    float* var;                   // moments: [rows][T][D] or NULL
    int32_t* saturated;           // eval: [rows][D] or NULL
    float* sat_frac;              // moments: [rows][D] or NULL
    float* rmse;                  // eval: [rows][D] or NULL
    float* maxabs;                // eval: [rows][D] or NULL
    long long rows;
    int S, D, Kb, T, nc;
};

struct MotionFitArgs {
    const float* traj;            // [rows][T][D]
    const float* pinv;            // [Kb][T]
    const float* scale;           // [P] or NULL
    const float* shift;           // [P] or NULL
    float* params;                // [rows][P]
    long long rows;
    int D, Kb, T;
};

// dynamic LDS of the two kernels, in bytes (the layout is lds_layout's in avae_motion.hip)
inline size_t motion_lds_bytes(int D, int Kb, int T, int nc, bool moments, bool ref_params) {
    const size_t ts = motion_slab(D, Kb, T), kp = motion_pad(Kb), tile = (size_t)kMotionRows * D * kp;
    size_t f = ts * kp + ts * nc + tile * (moments || ref_params ? 2 : 1) + (size_t)(moments ? 1 : kMotionRows) * D * nc;
    f = (f + 1) & ~(size_t)1;                                                               // the reduction buffer is 8-byte aligned
    return f * 4 + (moments ? (size_t)kMotionThreads * 8 : (size_t)kMotionRows * kMotionThreads * 4);
}

void launch_motion_eval(const MotionArgs& a, hipStream_t s);
void launch_motion_moments(const MotionArgs& a, hipStream_t s);
void launch_motion_fit(const MotionFitArgs& a, hipStream_t s);

}  // namespace avae
