// Sigma-lognormal strokes (avae_lognormal_eval / avae_lognormal_sample / avae_lognormal_fit; include/avae.h):
// the launch shapes and the kernel arguments shared by the host (avae_host.hip) and the kernels (avae_lognormal.hip).
//
// THE COMPONENT (all three kernels; plain fp32 operations in the order written, no fma; logf, expf, erff and sincosf stand for
// the double-precision function of the float argument rounded once to float -- the correctly rounded result, which no math
// library's choice within its ulp can change; z / sigma, up to 30, multiplies such a choice in the exponent).  With p = (D, t0, mu, sigma, ths, the) and the time t = (float)k * dt:
//     tau = t - t0;  sg = fmaxf(sigma, 1e-6f);  on = tau >= 1e-6f;  tc = fmaxf(tau, 1e-6f);  z = (logf(tc) - mu) / sg
//     u = on ? expf(-(z * z) * 0.5f) / ((sg * 2.5066282746f) * (tc + 1e-5f)) : 0;   amp = D * u;   a = fabsf(amp)
//     E = erff(z);  phi = ths + ((the - ths) * 0.5f) * (1.0f + E);  (sn, cs) = sincosf(phi);  the component adds (a * cs, a * sn)
//   v_k = the sum of these over c = 0 .. count - 1, c ascending, from (0, 0).
//   Its Jacobian (k_lognormal_fit), with s = +1, -1 or 0 the sign of amp, q = the - ths and, per parameter, da and dphi:
//     D:      da = s * u                                                      dphi = 0
//     t0:     da = (s * amp) * (1 / (tc + 1e-5f) + z / (sg * tc))             dphi = K * (on ? 1 / (sg * tc) : 0)
//     mu:     da = ((s * amp) * z) / sg                                       dphi = K * (1 / sg)
//     sigma:  da = ((s * amp) * (z * z - 1)) / sg                             dphi = K * (z / sg)
//     ths:    da = 0                                                          dphi = 1 - H
//     the:    da = 0                                                          dphi = H
//     K = -(q * 0.5641895835f) * expf(-(z * z)),  H = 0.5f * (1 + E);   dv = (da * cs - (a * sn) * dphi,  da * sn + (a * cs) * dphi)
//
// k_lognormal_eval    one wave (64 threads) per stroke, lane = time point in chunks of 64; the row's parameters sit in LDS and are
//                     read as broadcasts.  Per chunk: the lane's v_k (0 for k >= T); THE SCAN over the 64 lanes, for off = 1, 2, 4,
//                     8, 16, 32:  x_i <- x_i + x_(i - off) for every i >= off at once;  s_k = carry + x_k (carry: 0 for the first
//                     chunk, then s at lane 63 of the chunk before);  path_k = start + dt * s_k.  A row with a non-finite start or
//                     parameter (c < count) is NaN everywhere.
// k_lognormal_sample  one wave per (row, sample).  Lane c < count draws its Philox block and writes the perturbed component to LDS
//                     (n_i = normal_i / 3.0f;  D' = D + (n0 * amplitude) * D;  ths' = ths + n1 * angle;  the' = (the + n1 * angle)
//                     + (n2 * straightness) * (the - ths));  the stroke is then k_lognormal_eval's, bit for bit.  With shift_mean:
//                     every lane sums its own points (k = lane, lane + 64, ..., from 0, x and y apart), THE BUTTERFLY adds the 64
//                     sums (for off = 32, 16, 8, 4, 2, 1:  x_i <- x_i + x_(i xor off)), m = that / (float)T, and every point has m
//                     subtracted.  perturbed[n][s][c] = the component for c < count, zeros above.
// k_lognormal_fit     one workgroup of 256 threads per row, the whole Levenberg-Marquardt loop inside.  P = 6 * C parameters, index
//                     6 c + j.  A PASS over the stroke at parameters p goes through the time points in tiles of TT (below) points:
//       A. thread (tt, c): THE COMPONENT at k = tile + tt (and its Jacobian), into LDS
//       B. thread (xy):    for tt ascending:  v = sum_c (c ascending, from 0);  run = run + v;  pos = start + dt * run;  the errors
//                          e = (double)pos - (double)P_k  and  (double)v - (double)V_k,  V_k = (P_k - P_(k-1)) / dt in fp32
//                          (P_(-1) = start)
//          thread (i, xy): for tt ascending:  JV = dv_i;  runJ = runJ + JV;  JP = dt * runJ          (run, runJ carry over tiles)
//       C. per entry (i >= j) of M, of g and for the loss, one thread:  for tt ascending, for the rows (pos x, pos y, vel x, vel y)
//          with w = wp, wp, wv, wv:   M_ij += (w * (double)J_i) * (double)J_j;   g_i += (w * (double)J_i) * e;   L += (w * e) * e
//     The loop:  lam = 1e-3; per try:  a PASS with the Jacobian at p;  a masked parameter's rows and columns of M are 0 with 1 on the
//     diagonal and 0 in g;  d_i = M_ii of the free parameters, md = their maximum (i ascending, from 0);  M_ii += lam * d_i +
//     1e-12 * (md + 1) (free i);  Cholesky in double, column by column:  s = M_jj - L_j0^2 - .. (k ascending),  !(s > 0) rejects,
//     L_jj = sqrt(s),  L_ij = (M_ij - L_i0 L_j0 - ..) / L_jj;  y_i = (g_i - L_i0 y_0 - ..) / L_ii (i ascending);  x_i = (y_i -
//     L_(P-1)i x_(P-1) - ..) / L_ii (i descending, the subtrahends k descending);  a non-finite x rejects;  new_i = (float)((double)p_i
//     - x_i) for a free i (sigma: fminf(fmaxf(new, 1e-3f), 3.0f); then fmaxf(new, lo_j), fminf(new, hi_j) where given), p_i else;
//     a PASS without the Jacobian at new gives Ln;  Ln < L accepts (p = new, lam = max(lam / 3, 1e-9), and L - Ln < tol * L ends the
//     row with status 0), else lam = min(4 lam, 1e9) and p stays;  8 rejections in a row end it (status 0 when a step was
//     accepted before them: the damping has grown 65536-fold and nothing lowers the loss any more; status 2 when none ever was),
//     n_iters tries with status 1.
//   The size classes C <= 4, <= 8, <= 16 (template argument CC) set the LDS arrays: M is the lower triangle of 6 CC (6 CC + 1) / 2
//   doubles, a tile holds TT = 64, 32, 8 points (4 rows of 6 CC floats each).
//   Resources (the compiler's resource report): VGPRs / LDS bytes / scratch bytes
//       k_lognormal_eval 123 / 384 / 0        k_lognormal_sample 125 / 8576 / 0
//       k_lognormal_fit<4> 161 / 31696 / 0    k_lognormal_fit<8> 163 / 38280 / 0    k_lognormal_fit<16> 163 / 53240 / 0
//   (with the float functions of the math library in place of the double ones: 44, 66, 87, 89, 89 VGPRs)
// None of the kernels uses atomics or scratch memory or reads or writes anything of the handle.
#pragma once
#include "avae_latent_common.h"

namespace avae {

constexpr int kLnThreads = 64, kLnFitThreads = 256;
constexpr int kLnMaxC = 16, kLnMaxT = 1024, kLnMaxIters = 10000;
constexpr unsigned kLnSalt = 0x736c676eu;      // 'slgn'

struct LnEvalArgs {
    const float* params;          // [rows][C][6]
    const int* count;             // [rows]
    const float* start;           // [rows][2]
    float* path;                  // [rows][T][2]
    float* velocity;              // [rows][T][2] or NULL
    float dt;
    int rows, C, T;
};

struct LnSampleArgs {
    const float* params;          // [rows][C][6]
    const int* count;             // [rows]
    const float* start;           // [rows][2]
    float* strokes;               // [rows][S][T][2]
    float* perturbed;             // [rows][S][C][6] or NULL
    unsigned long long seed;
    unsigned row0;
    float dt, amplitude, angle, straightness;
    int rows, S, C, T, shift_mean;
};

struct LnFitArgs {
    const float* target;          // [rows][T][2]
    const float* init;            // [rows][C][6]
    const int* count;             // [rows]
    const float* start;           // [rows][2]
    const unsigned char* free_mask;   // NULL, [6] (free_per_row 0) or [rows][C][6] (free_per_row 1)
    const float* lo;              // NULL or [6]
    const float* hi;              // NULL or [6]
    float* params;                // [rows][C][6]
    double* loss0;                // [rows] or NULL
    double* loss;                 // [rows] or NULL
    int* iterations;              // [rows] or NULL
    int* accepted;                // [rows] or NULL
    int* status;                  // [rows] or NULL
    double wp, wv, tol;
    float dt;
    int rows, C, T, n_iters, free_per_row;
};

void launch_lognormal_eval(const LnEvalArgs& a, hipStream_t s);
void launch_lognormal_sample(const LnSampleArgs& a, hipStream_t s);
void launch_lognormal_fit(const LnFitArgs& a, hipStream_t s);

}  // namespace avae
