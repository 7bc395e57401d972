// Gradients through the writing chain (avae_stroke_render_vjp / avae_motion_fk_vjp / avae_motion_eval_vjp / avae_rows_adam;
// include/avae.h): the launch shapes and the kernel arguments shared by the host (avae_host.hip) and the
// kernels (avae_grad.hip).
//
// k_stroke_render_vjp  the forward's launch: one workgroup of 256 threads per row, and the forward itself first -- render_row of
//   avae_render_dev.h, the code k_stroke_render runs, so the forward outputs it writes on request are that kernel's bits and the
//   decisions of the reverse pass (inked list, nearest segment, zone) are made on the forward's own numbers.  Then, with the
//   segment records, the image and the inked list still in LDS:
//   a. g_pix = (g_image + (g_img_l2 * (image - target)) / img_l2) * (1 / ss^2) replaces the image in LDS (the second term only
//      where img_l2 != 0); B = ss^2 sum |g_pix| / delta through THE TREE bounds every sum of c. below.
//   b. the first index of the largest and of the smallest cu and cv (exact comparisons with the box, THE TREE with min).
//   c. the forward's step 5 again, a thread per sub-row of an inked pixel: the running minimum by `d2 < m` (strict, so the first
//      segment that attains it is kept, and m is fminf's), then per sample in the open zone 0 < x < 1 the foot parameter tau and the
//      offset e of the kept segment recomputed as seg_dist2 forms them, d = sqrtf(m), n = e / d (0 where d == 0),
//      g_d = -g_pix / delta, g_s = g_d n; endpoint A gets -((1 - tau) g_s) and B -(tau g_s) per axis, and the thread keeps
//      sum g_s (2), sum (g_s.u alpha_b - g_s.v alpha_a) and sum -(((r - d) / delta) / delta) g_pix.
//      Every one of these sums is a 64-bit fixed-point integer: a term x becomes rint(x * 2^(60 - e)), B = f * 2^e with f in
//      [0.5, 1), the multiplication exact in double.  |term| <= |g_pix| / delta and a sum has at most ss^2 terms per pixel, so
//      |sum| < 2^60: three bits of headroom.  The per-point sums are LDS integer atomics (ds_add_u64), the four window sums a
//      thread's own registers and then four LDS atomics per thread: integer addition commutes exactly, so the bits do not depend
//      on the order the hardware takes.  No floating-point atomic anywhere.
//   d. thread t, t + 256, ... finishes point t: g_c = (float)(sum * 2^(e - 60)), + g_ctr / 2 at the first argmax and again at the
//      first argmin of its axis, +- (1 + margin) g_W at those of the longer axis (u on a tie), g_W = sum_W + g_delta / (H ss);
//      grad_path_t = fma(g_cv, v, g_cu * u) per coordinate, then fma(k_t, n, .) with k_t = (g_height_l2 * (n.p_t - height)) /
//      height_l2 where height_l2 != 0.
//   LDS: the forward's + 16 T bytes + 32 (15.7 KiB at T = 100, H = 28: ten workgroups' worth of a CU's 160 KiB, the 32 waves of a CU
//   bound it to 8; 74.8 KiB at T = 1024, H = 64, which the launcher opts in for).
// k_motion_fk_vjp      k_motion_fk's tile shape: one thread per (row, t), 256 per workgroup, angles in and gradients out through
//   LDS rows of odd length D | 1.  The chain inwards exactly as k_motion_fk (sines and cosines kept in LDS), then outwards with the
//   tip v and the cotangent h: per joint j  w = R_j^T (v - p_j), h = R_j^T h  (frame j, transposed products in the forward's
//   association), grad_q_j = ((a x w) . h) -- (a_j x (tip - o_j)) . g written in joint j's frame --, then v = Rot(a_j, -q_j) w and
//   h = Rot(a_j, -q_j) h.  Six floats of state: the Jacobian is never formed.
// k_motion_eval_vjp    k_motion_fit's tile shape: a workgroup per tile of kMotionRows rows, thread tid owns parameters tid, tid +
//   256, ...; per time slab of kFitSlab points phi (transposed) and the rows' masked gradients are staged in LDS.  With limits the
//   unclamped q is formed as k_motion_eval forms it (theta = fma(params, scale, shift), fma chain over k from 0, the anchor terms
//   in index order) and the gradient of a point passes where lo <= q <= hi.  One fma chain over t per (row, d, k), times scale.
// k_rows_adam          a workgroup per row, thread i owns elements i, i + 256, ... (n <= 1024): the best-so-far copy, the finite
//   test, |g|^2 (fma chain per thread, THE TREE), the update with the row's own step count.
// No kernel reads or writes anything of the handle; none uses scratch or a floating-point atomic.
#pragma once
#include "avae_motion.h"
#include "avae_render.h"

namespace avae {

struct RenderVjpArgs {
    RenderArgs f;                 // the forward's arguments; its outputs are optional here
    const float* g_image;         // [rows][H * H] or NULL
    const float* g_img_l2;        // [rows] or NULL
    const float* g_height_l2;     // [rows] or NULL
    float* grad_path;             // [rows][T][3]
    float* objective;             // [rows] or NULL: g_img_l2 img_l2 + g_height_l2 height_l2
};

// dynamic LDS of k_stroke_render_vjp in floats: the forward's, then the per-point sums of u and v (64 bit each) and 4 window sums
struct RenderVjpLds { int accu, accv, slots, floats; };
__host__ __device__ inline RenderVjpLds render_vjp_lds(int T, int H) {
    RenderVjpLds l;
    l.accu = (render_lds(T, H).floats + 1) & ~1;
    l.accv = l.accu + 2 * T;
    l.slots = l.accv + 2 * T;
    l.floats = l.slots + 8;
    return l;
}
inline size_t render_vjp_lds_bytes(int T, int H) { return (size_t)render_vjp_lds(T, H).floats * 4; }

struct FkVjpArgs {
    const float* traj;            // [rows][T][D]
    const float* frames;          // [D + 1][3][4]
    const float* axes;            // [D][3]
    const float* grad_path;       // [rows][T][3]
    float* grad_traj;             // [rows][T][D]
    long long points;             // rows * T
    int D;
};

struct MotionVjpArgs {
    const float* params;          // [rows][P]
    const float* phi;             // [T][Kb]
    const float* scale;           // [P] or NULL
    const float* shift;           // [P] or NULL
    const float* limits;          // [D][2] or NULL
    const float* gain;            // [T][nc] or NULL
    const float* target;          // [rows][D][nc] or NULL
    const float* grad_traj;       // [rows][T][D]
    float* grad_params;           // [rows][P]
    long long rows;
    int D, Kb, T, nc;
};

constexpr int kRowsAdamThreads = 256, kRowsAdamMaxN = 1024;

struct RowsAdamArgs {
    float* x;                     // [P][n]
    const float* g;               // [P][n]
    float* m;                     // [P][n]
    float* v;                     // [P][n]
    int32_t* t;                   // [P]
    int32_t* status;              // [P]
    const float* cost;            // [P] or NULL
    float* best_cost;             // [P] (with cost)
    float* best_x;                // [P][n] (with cost)
    int n;
    float lr, beta1, beta2, eps, max_norm;   // max_norm <= 0: no clipping
};

void launch_stroke_render_vjp(const RenderVjpArgs& a, long long rows, hipStream_t s);
void launch_motion_fk_vjp(const FkVjpArgs& a, hipStream_t s);
void launch_motion_eval_vjp(const MotionVjpArgs& a, hipStream_t s);
void launch_rows_adam(const RowsAdamArgs& a, long long rows, hipStream_t s);

}  // namespace avae
