// Pose, Jacobian and inverse kinematics of a serial chain (avae_motion_pose / avae_motion_ik; include/avae.h):
// the launch shapes and the kernel arguments shared by the host (avae_host.hip) and the kernels (avae_ik.hip).
//
// THE WALK (both kernels, one lane per pose, base to tip; plain fp32 multiplies and adds in the order written, no fma; sincosf is
// the precise one).  R = I, p = 0.  For j = 0 .. D - 1, with frame j = (F | f) and axis a = axes[j]:
//     p[r]    = (((R[r][0] f[0] + R[r][1] f[1]) + R[r][2] f[2]) + p[r])              (the old R)
//     R[r][c] = (R[r][0] F[0][c] + R[r][1] F[1][c]) + R[r][2] F[2][c]
//     o_j = p,  z_j[r] = (R[r][0] a[0] + R[r][1] a[1]) + R[r][2] a[2]
//     every row r of R is turned by Rodrigues' formula:  x = r x a (two products and a difference per component),
//     k = ((r[0] a[0] + r[1] a[1]) + r[2] a[2]) (1 - c),  r <- (r c + x s) + a k,  (s, c) = sincosf(q_j)
//   then frame D the same way (p first, then R).  Jacobian column j:  d = p - o_j,  J_v = z_j x d (as above),  J_w = z_j.
//
// k_motion_pose   one thread per (row, t), 256 per workgroup, a workgroup per tile of 256 consecutive points (grid-stride); the
//                 tile's angles come in through LDS as in k_motion_fk (rows of odd length D | 1), position and rotation (12 floats a
//                 point) go out through LDS with consecutive lanes on consecutive floats; a Jacobian column is stored from
//                 registers (6 floats a lane, stride 6 D between lanes).  The chain constants sit in LDS and are read as broadcasts.
// k_motion_ik     one lane per row, 64 per workgroup (one wave: 4096 rows are 64 workgroups on 64 CUs, not 16 full ones); the lane
//                 walks its row's T points with q, o_j / J_v, z_j, M and L in registers.  At a point, with the target g and
//                 k = 0, 1, ...:
//     THE WALK at q;  e_p = g - p;  with a goal G:  e_w = 0.5 * sum_i R[:, i] x G[:, i]  (i ascending, from the first term)
//     residual = sqrtf((e_p0^2 + e_p1^2) + e_p2^2), rot_residual the same of e_w
//     status 0 when residual < tol (and rot_residual < rot_tol); else status 1 when k == n_iters; else
//     M[i][j] = sum_c J[i][c] J[j][c] (c ascending from the first product), i >= j, then M[i][i] + damping * damping
//     Cholesky, column by column:  s = M[j][j] - L[j][0]^2 - ... (k ascending);  !(s > 0) -> status 2;  L[j][j] = sqrtf(s);
//         L[i][j] = (M[i][j] - L[i][0] L[j][0] - ...) / L[j][j]
//     y[i] = (e[i] - L[i][0] y[0] - ...) / L[i][i]  (i ascending);   x[i] = (y[i] - L[m-1][i] x[m-1] - ...) / L[i][i]  (i descending,
//         the subtrahends k descending)
//     dq[c] = sum_i J[i][c] x[i] (i ascending);  s = fmaxf(.. fmaxf(fmaxf(0, |dq[0]|), |dq[1]|) ..) (C's fmaxf: a NaN operand is
//         dropped);  s > max_step:  dq[c] = dq[c] * (max_step / s)
//     n[c] = q[c] + dq[c];  a step is committed only when every n[c] is finite:  !(sum_c n[c] * 0 == 0) -> status 2 with q as it
//         was;  else  q[c] = n[c],  with limits  q[c] = fminf(fmaxf(n[c], lo[c]), hi[c])
//   sqrtf and the divisions are IEEE.  Status 2 is "the solve failed", by a pivot or by a non-finite step (damping^2 that underflows,
//   a target so far away that M^-1 e overflows): the point ends with the last good q, its residuals and the steps taken so far, and
//   the next point starts from that q.  A non-finite target point: NaN angles and residuals, 0 iterations, status 3, the carried q
//   untouched; a non-finite seed: that for every point of the row.  So the carried q is finite whenever the seed is.  A lane that is
//   done at a point sits out the wave's remaining trips with its registers unchanged.
//   D and m (3 without a goal, 6 with one) are template arguments, so that every array is indexed at compile time: the classes
//   D <= 4, <= 8, <= 16 (a joint c >= D is skipped by a uniform branch) times m = 3, 6.
//   Resources (k_motion_ik<DC, m>, the compiler's resource report): VGPRs / LDS bytes / scratch bytes
//       <4, 3> 112 / 320 / 0    <4, 6> 136 / 320 / 0    <8, 3> 158 / 592 / 0    <8, 6> 172 / 592 / 0
//       <16, 3> 248 / 1136 / 0  <16, 6> 249 / 1136 / 0  (one wave per SIMD at 64 threads a workgroup: up to 512 registers a lane)
//   k_motion_pose<DC>:  <4> 118 / 17696 / 0    <8> 180 / 22032 / 0    <16> 256 + 30 AGPRs / 30704 / 0
//   The chain constants are read from LDS inside the walk (a compiler barrier per joint keeps the loads from being hoisted out of
//   the solver's loops, where they would pin 15 registers a joint and spill: 2 KiB of scratch at DC = 16 without it).
// Neither kernel uses atomics or scratch memory or reads or writes anything of the handle.
#pragma once
#include "avae_latent_common.h"
#include "avae_render.h"

namespace avae {

constexpr int kIkThreads = 64, kPoseThreads = 256;
constexpr int kIkMaxD = kFkMaxD, kIkMaxT = kRenderMaxT, kIkMaxIters = 1000;

struct PoseArgs {
    const float* traj;            // [rows][T][D]
    const float* frames;          // [D + 1][3][4]
    const float* axes;            // [D][3]
    float* position;              // [rows][T][3] or NULL
    float* rotation;              // [rows][T][3][3] or NULL
    float* jacobian;              // [rows][T][6][D] or NULL
    long long points;             // rows * T
    int D;
};

struct IkArgs {
    const float* path;            // [rows][T][3]
    const float* frames;          // [D + 1][3][4]
    const float* axes;            // [D][3]
    const float* seed;            // [rows][D]
    const float* orient;          // NULL or [orient_rows][3][3]
    const float* limits;          // NULL or [D][2]
    float* traj;                  // [rows][T][D]
    float* residual;              // [rows][T] or NULL
    float* rot_residual;          // [rows][T] or NULL
    int* iterations;              // [rows][T] or NULL
    int* status;                  // [rows][T] or NULL
    float tol, rot_tol, damping, max_step;
    int rows, T, D, n_iters, orient_per_row;
};

void launch_motion_pose(const PoseArgs& a, hipStream_t s);
void launch_motion_ik(const IkArgs& a, hipStream_t s);

}  // namespace avae
