// Joint-trajectory synthesis by iLQR on a double-integrator joint model (avae_motion_track; include/avae.h):
// the launch shape, the workspace layout and the kernel arguments shared by the host (avae_host.hip) and the kernel
// (avae_track.hip).  tests/track_reference.py restates everything below.
//
// Row r, D joints, T points, n = 2 D.  State x_t = (q_t, v_t), t < T; control u_t, t < T - 1;  q_(t+1) = q_t + dt v_t,
// v_(t+1) = v_t + dt u_t  (each one product and one sum, in double);  x_0 = (init[0], 0).
// THE FIRST CONTROLS (double, from the float init):  v0_0 = 0,  v0_t = (init_t - init_(t-1)) / dt,  u_t = (v0_(t+1) - v0_t) / dt;
//   the first trajectory is their rollout from x_0.
// THE POINT at t sees qf = (float) q_t and nothing else of the state.  THE WALK of avae_ik.h at qf gives the tip p and the linear
//   Jacobian rows J_v (fp32), with one difference: sin and cos are the double-precision functions of the float angle, rounded
//   once (the correctly rounded floats but for double's own last bit).  Four tries multiply what a float math library picks
//   within its ulp until two correct implementations stand 6x apart in the cost (5.7e-7 against 9.3e-8 on the first GPU run; the
//   NumPy restatement moved from 9.3e-8 to 4.0e-7 when its own sines were exchanged): rounded once, kernel and restatement walk
//   the same bits, as in avae_lognormal.h.  With the target g = path[t], the track weights w (float) and wd = (double) w:
//     e_r = (double) p_r - (double) g_r;   track = ((wd_0 e_0)^2 + (wd_1 e_1)^2) + (wd_2 e_2)^2;   sq = (e_0^2 + e_1^2) + e_2^2
//     with limits:  viol_j = qf_j > hi_j ? qf_j - hi_j : (qf_j < lo_j ? qf_j - lo_j : 0)  (in double from the floats);
//         pen = sum_j viol_j^2 (j ascending from 0);  c = track + wl pen;   without:  c = track
//     t < T - 1:  eff = sum_i u_i (sum_j Se[i][j] u_j)  (both ascending from 0);  c = c + eff
//   Se = R sum_k E[k][i] E[k][j]  (k ascending from 0, double from the float E), or R on the diagonal and 0 elsewhere without E.
//   The linearisation (fp32; ww_r = w_r w_r,  ew_r = ww_r (p_r - g_r),  J_ri = J_v[r][i]):
//     l_q[i]     = 2 ((J_0i ew_0 + J_1i ew_1) + J_2i ew_2);                   a violated joint:  + (2 wl) viol_i  (viol in float)
//     l_qq[i][j] = 2 ((J_0i (ww_0 J_0j) + J_1i (ww_1 J_1j)) + J_2i (ww_2 J_2j)),  i >= j;   a violated joint:  l_qq[i][i] + 2 wl
// THE COST  lane l sums c_t over t = l, l + 64, ... ascending from 0; J is the butterfly of the 64 sums (x = x + x of lane ^ off,
//   off = 32, 16, .., 1: every lane gets the same bits); the sum of sq the same way; track_rmse = sqrt(sum sq / T).
// THE BACKWARD PASS (double; a = V_x[0:D], b = V_x[D:n], P, Q, S the qq, qv and vv blocks of V_xx; every sum over an index ascending
//   from 0).  At t = T - 1:  V_x = (l_q, 0), V_xx = l_qq in the qq block and 0 elsewhere.  Then t = T - 2 .. 0:
//     Q_x  = (l_q + a,  dt a + b);      Q_u[i] = 2 (sum_j Se[i][j] u_t[j]) + dt b[i]
//     Q_xx:  qq = l_qq + P;   qv[i][j] = dt P[i][j] + Q[i][j];   vq = qv^T;   vv[i][j] = (dt qv[i][j] + dt Q[j][i]) + S[i][j]
//     Q_ux:  [i][j] = dt Q[j][i]  (j < D);    [i][D + j] = dt (dt Q[j][i] + S[i][j])
//     Q_uu[i][j] = (2 Se[i][j] + (dt dt) S[i][j]) + (i == j ? lam : 0)
//     Q_uu = L L^T, column by column:  s_i = Q_uu[i][j] - L[i][0] L[j][0] - ... (k ascending), i >= j;  !(s_j > 0) rejects the try;
//         L[j][j] = sqrt(s_j),  L[i][j] = s_i / L[j][j]
//     for each of the n + 1 right-hand sides y = Q_u, Q_ux[:, c]:  forward (i ascending, the subtrahends k ascending), back (i
//         descending, k descending), as in avae_ik.h;  k = -x,  K[:, c] = -x.  A gain that is not finite, as double or as float,
//         rejects the try.  The floats go to the workspace, the recursion goes on with the doubles.
//     M[i][c] = (sum_j Q_uu[i][j] K[j][c]) + Q_ux[i][c],   m[i] = (sum_j Q_uu[i][j] k[j]) + Q_u[i]
//     V_x[r]     = (Q_x[r] + sum_i K[i][r] m[i]) + sum_i Q_ux[i][r] k[i]
//     V_xx[r][c] = (Q_xx[r][c] + sum_i K[i][r] M[i][c]) + sum_i Q_ux[i][r] K[i][c],   then  V_xx[r][c] = 0.5 (V_xx[r][c] + V_xx[c][r])
// THE FORWARD PASS (double, the float gains widened):  x'_0 = x_0;
//     u'_t[i] = (u_t[i] + k_t[i]) + K_t[i][0] dx_0 + ... + K_t[i][n - 1] dx_(n-1),  dx = x'_t - x_t  (c ascending);  x'_(t+1) as above.
// THE LOOP:  J at the first trajectory is cost0.  lam = lam0.  A try (while tries < n_iters):  backward at lam; if it was not
//   rejected, forward and J' = THE COST of x', u'.  J' < J accepts: the trajectory is x', u', lam = max(lam / factor, lam_min), and
//   the row ends with status 0 when J - J' < tol J (the old J; strict).  Otherwise lam = lam factor, and the row ends when
//   lam > lam_max: status 0 if a try was ever accepted, else 2.  Status 1: n_iters tries made.  T = 1: no try, status 0.
//   A non-finite path point, init value or (used) limit: status 3, NaN in traj, controls, cost0, cost and track_rmse, 0 tries.
//
// k_motion_track<DC>  one workgroup of one wave (64 lanes) per row, the whole loop inside one launch.  Points (THE POINT, the
//   linearisation): one lane per time point, grid-striding over T inside the wave, the chain constants in LDS as in k_motion_pose.
//   Backward: sequential in t; the lanes share the entries of V_xx, Q_xx, Q_ux, Q_uu, M in LDS; the Cholesky as in k_lognormal_fit
//   (a lane per row of the column), the n + 1 solves a lane per right-hand side, in place in LDS.  Forward: lane i carries q'_i, v'_i
//   and u'_i; dx goes round by wave shuffles, the step's gains and old state are loaded a step ahead.
//   The workspace of a row (track_row_bytes, a multiple of 256):  x [2][T][n] and u [2][T][D] in double (the trajectory and the
//   candidate, swapped on acceptance), then in float the gains [T][D][n + 1] (k first), l_q [T][D] and l_qq [T][D (D + 1) / 2].
//   A workgroup reads back only what it wrote itself.  Vector stores and plain C++ only.
//   D classes <= 4, <= 8, <= 16 (compile-time indexed walk; a joint c >= D is skipped by a uniform branch).
//   Resources (k_motion_track<DC>, the compiler's resource report): VGPRs / LDS bytes / scratch bytes
//       <4> 255 + 2 AGPRs / 2760 / 0    <8> 256 + 40 AGPRs / 9816 / 0    <16> 256 + 147 AGPRs / 36984 / 0
//   One wave per SIMD, so four rows a CU and 1024 rows on the device at a time; LDS would allow 16 rows a CU at D <= 8 and four
//   at D = 16.  Asking the compiler for two waves per SIMD spills (12 bytes of scratch a lane at DC = 4, 152 at DC = 8): open.
// No atomics, no scratch memory, nothing of the handle is read or written.
#pragma once
#include "avae_latent_common.h"
#include "avae_ik.h"

namespace avae {

constexpr int kTrackThreads = 64;
constexpr int kTrackMaxD = kIkMaxD, kTrackMaxT = kIkMaxT, kTrackMaxIters = 1000;

// bytes of one row's workspace: 8 (2 T n + 2 T D) + 4 T (D (n + 1) + D + D (D + 1) / 2) = T (10 D^2 + 58 D), rounded up to 256
inline size_t track_row_bytes(int T, int D) {
    const size_t b = (size_t)T * (size_t)(10 * D * D + 58 * D);
    return (b + 255) / 256 * 256;
}

struct TrackArgs {
    const float* path;            // [rows][T][3]
    const float* init;            // [rows][T][D]
    const float* frames;          // [D + 1][3][4]
    const float* axes;            // [D][3]
    const float* effort;          // NULL or [D][D]
    const float* limits;          // NULL (no limit term) or [D][2]
    unsigned char* workspace;     // [rows][row_bytes]
    float* traj;                  // [rows][T][D]
    float* controls;              // [rows][T - 1][D] or NULL
    double* cost0;                // [rows] or NULL
    double* cost;                 // [rows] or NULL
    float* rmse;                  // [rows] or NULL
    int* iterations;              // [rows] or NULL
    int* accepted;                // [rows] or NULL
    int* status;                  // [rows] or NULL
    double lam0, factor, lam_min, lam_max, tol;
    size_t row_bytes;
    float dt, w[3], R, limit_weight;
    int rows, T, D, n_iters;
};

void launch_motion_track(const TrackArgs& a, hipStream_t s);

}  // namespace avae
