// Joint-trajectory synthesis by iLQR (avae_track.h, include/avae.h): k_motion_track.
#include "avae_device.h"
#include "avae_track.h"
#include "avae_walk.h"

namespace avae {

namespace {

// Every operation below is the one avae_track.h writes, in its order: tests/track_reference.py restates them one by one.
#pragma clang fp contract(off)

static_assert(kTrackThreads == 64, "one wave per row: the forward pass passes dx round by wave shuffles");

template <int DC>
struct TrackLds {
    static constexpr int N = 2 * DC;
    double V[N * N];                   // V_xx, rows of n = 2 D
    double Qxx[N * N];
    double Qux[DC * N];
    double G[DC * (N + 1)];            // rows of n + 1: k first, then K (the solves run in place)
    double M[DC * (N + 1)];            // rows of n + 1: m first, then M
    double Quu[DC * DC], L[DC * DC], Se[DC * DC];
    double vx[N], Qx[N], Qu[DC], col[DC];
    float frames[(DC + 1) * 12], axes[DC * 3], lim[DC * 2];
    int flag;
};

// THE POINT for every t (a lane per point) and THE COST; with LIN also the linearisation into lq, lqq
template <int DC, bool LIN>
__device__ __forceinline__ double point_pass(const TrackArgs& a, TrackLds<DC>& s, const float* path, const double* x, const double* u,
                                             float* lq, float* lqq, double& sq_sum) {
    const int D = a.D, T = a.T, n = 2 * D, tri = D * (D + 1) / 2, tid = threadIdx.x;
    const bool lim = a.limits != nullptr;
    const float w0 = a.w[0], w1 = a.w[1], w2 = a.w[2], wl = a.limit_weight;
    double part = 0.0, part2 = 0.0;
    for (int t = tid; t < T; t += kTrackThreads) {
        double eff = 0.0;                                       // (ahead of the walk: the controls' registers are free again in it)
        if (t < T - 1) {
            double uu[DC];
#pragma unroll
            for (int c = 0; c < DC; ++c) uu[c] = c < D ? u[(size_t)t * D + c] : 0.0;
#pragma unroll
            for (int i = 0; i < DC; ++i) {
                if (i < D) {
                    double r = 0.0;
#pragma unroll
                    for (int j = 0; j < DC; ++j)
                        if (j < D) r = r + s.Se[i * D + j] * uu[j];
                    eff = eff + uu[i] * r;
                }
            }
        }
        float q[DC];
#pragma unroll
        for (int c = 0; c < DC; ++c) q[c] = c < D ? (float)x[(size_t)t * n + c] : 0.0f;
        Walk<DC> w;
        walk<DC, true>(s.frames, s.axes, D, q, w);
        const float g0 = path[3 * t], g1 = path[3 * t + 1], g2 = path[3 * t + 2];
        const double e0 = (double)w.p[0] - (double)g0, e1 = (double)w.p[1] - (double)g1, e2 = (double)w.p[2] - (double)g2;
        const double we0 = (double)w0 * e0, we1 = (double)w1 * e1, we2 = (double)w2 * e2;
        double c_t = (we0 * we0 + we1 * we1) + we2 * we2;
        part2 = part2 + ((e0 * e0 + e1 * e1) + e2 * e2);
        if (lim) {
            double pen = 0.0;
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                if (c < D) {
                    const float lo = s.lim[2 * c], hi = s.lim[2 * c + 1];
                    const double v = q[c] > hi ? (double)q[c] - (double)hi : (q[c] < lo ? (double)q[c] - (double)lo : 0.0);
                    pen = pen + v * v;
                }
            }
            c_t = c_t + (double)wl * pen;
        }
        if (t < T - 1) c_t = c_t + eff;
        part = part + c_t;
        if (LIN) {
            const float ww0 = w0 * w0, ww1 = w1 * w1, ww2 = w2 * w2, twl = 2.0f * wl;
            const float ew0 = ww0 * (w.p[0] - g0), ew1 = ww1 * (w.p[1] - g1), ew2 = ww2 * (w.p[2] - g2);
            jacobian_columns<DC>(D, w);
            float* lq_t = lq + (size_t)t * D;
            float* lqq_t = lqq + (size_t)t * tri;
#pragma unroll
            for (int i = 0; i < DC; ++i) {
                if (i < D) {
                    float v = 2.0f * ((w.o[i][0] * ew0 + w.o[i][1] * ew1) + w.o[i][2] * ew2);
                    float viol = 0.0f;
                    if (lim) {
                        const float lo = s.lim[2 * i], hi = s.lim[2 * i + 1];
                        viol = q[i] > hi ? q[i] - hi : (q[i] < lo ? q[i] - lo : 0.0f);
                    }
                    if (viol != 0.0f) v = v + twl * viol;
                    lq_t[i] = v;
#pragma unroll
                    for (int j = 0; j <= i; ++j) {
                        float h = 2.0f * ((w.o[i][0] * (ww0 * w.o[j][0]) + w.o[i][1] * (ww1 * w.o[j][1])) + w.o[i][2] * (ww2 * w.o[j][2]));
                        if (j == i && viol != 0.0f) h = h + twl;
                        lqq_t[i * (i + 1) / 2 + j] = h;
                    }
                }
            }
        }
    }
    // THE BUTTERFLY: every lane gets the sum
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        part = part + __shfl_xor(part, off, kTrackThreads);
        part2 = part2 + __shfl_xor(part2, off, kTrackThreads);
    }
    sq_sum = part2;
    return part;
}

// THE BACKWARD PASS at lam: the float gains into `gains`; false when the try is rejected (uniform over the wave)
template <int DC>
__device__ __forceinline__ bool backward_pass(const TrackArgs& a, TrackLds<DC>& s, const double* u, const float* lq, const float* lqq,
                                              float* gains, double lam) {
    const int D = a.D, T = a.T, n = 2 * D, ng = n + 1, tri = D * (D + 1) / 2, tid = threadIdx.x;
    const double dt = (double)a.dt, dt2 = dt * dt;
    {
        const float* lqq_t = lqq + (size_t)(T - 1) * tri;
        for (int e = tid; e < n * n; e += kTrackThreads) {
            const int r = e / n, c = e - r * n;
            double v = 0.0;
            if (r < D && c < D) {
                const int i = r > c ? r : c, j = r > c ? c : r;
                v = (double)lqq_t[i * (i + 1) / 2 + j];
            }
            s.V[e] = v;
        }
        if (tid < n) s.vx[tid] = tid < D ? (double)lq[(size_t)(T - 1) * D + tid] : 0.0;
        if (tid == 0) s.flag = 0;
    }
    __syncthreads();
    for (int t = T - 2; t >= 0; --t) {
        const float* lq_t = lq + (size_t)t * D;
        const float* lqq_t = lqq + (size_t)t * tri;
        const double* u_t = u + (size_t)t * D;
        float* g_t = gains + (size_t)t * D * ng;
        // Q_xx, Q_ux, Q_uu, Q_x, Q_u
        for (int e = tid; e < n * n; e += kTrackThreads) {
            const int r = e / n, c = e - r * n;
            const int i = r < D ? r : r - D, j = c < D ? c : c - D;
            double v;
            if (r < D) {
                if (c < D) {
                    const int hi = i > j ? i : j, lo = i > j ? j : i;
                    v = (double)lqq_t[hi * (hi + 1) / 2 + lo] + s.V[i * n + j];
                } else {
                    v = dt * s.V[i * n + j] + s.V[i * n + D + j];
                }
            } else {
                if (c < D) v = dt * s.V[j * n + i] + s.V[j * n + D + i];
                else v = (dt * (dt * s.V[i * n + j] + s.V[i * n + D + j]) + dt * s.V[j * n + D + i]) + s.V[(D + i) * n + D + j];
            }
            s.Qxx[e] = v;
        }
        for (int e = tid; e < D * n; e += kTrackThreads) {
            const int i = e / n, c = e - i * n;
            s.Qux[e] = c < D ? dt * s.V[c * n + D + i] : dt * (dt * s.V[(c - D) * n + D + i] + s.V[(D + i) * n + c]);
        }
        for (int e = tid; e < D * D; e += kTrackThreads) {
            const int i = e / D, j = e - i * D;
            double v = 2.0 * s.Se[e] + dt2 * s.V[(D + i) * n + D + j];
            if (i == j) v = v + lam;
            s.Quu[e] = v;
            s.L[e] = v;
        }
        if (tid < n) s.Qx[tid] = tid < D ? (double)lq_t[tid] + s.vx[tid] : dt * s.vx[tid - D] + s.vx[tid];
        if (tid >= 32 && tid < 32 + D) {
            const int i = tid - 32;
            double r = 0.0;
            for (int j = 0; j < D; ++j) r = r + s.Se[i * D + j] * u_t[j];
            s.Qu[i] = 2.0 * r + dt * s.vx[D + i];
        }
        __syncthreads();
        // Q_uu = L L^T
        for (int j = 0; j < D; ++j) {
            if (tid >= j && tid < D) {
                double v = s.L[tid * D + j];
                for (int k = 0; k < j; ++k) v = v - s.L[tid * D + k] * s.L[j * D + k];
                s.col[tid] = v;
            }
            __syncthreads();
            const double piv = s.col[j];
            if (!(piv > 0.0)) return false;
            const double d = sqrt(piv);
            if (tid >= j && tid < D) s.L[tid * D + j] = tid == j ? d : s.col[tid] / d;
            __syncthreads();
        }
        // the n + 1 solves, a lane per right-hand side
        if (tid < ng) {
            const int c = tid;
            for (int i = 0; i < D; ++i) {
                double v = c == 0 ? s.Qu[i] : s.Qux[i * n + c - 1];
                for (int k = 0; k < i; ++k) v = v - s.L[i * D + k] * s.G[k * ng + c];
                s.G[i * ng + c] = v / s.L[i * D + i];
            }
            for (int i = D - 1; i >= 0; --i) {
                double v = s.G[i * ng + c];
                for (int k = D - 1; k > i; --k) v = v - s.L[k * D + i] * s.G[k * ng + c];
                s.G[i * ng + c] = v / s.L[i * D + i];
            }
            bool bad = false;
            for (int i = 0; i < D; ++i) {
                const double g = -s.G[i * ng + c];
                const float gf = (float)g;
                s.G[i * ng + c] = g;
                g_t[i * ng + c] = gf;
                bad = bad || !isfinite(g) || !isfinite(gf);
            }
            if (bad) s.flag = 1;
        }
        __syncthreads();
        if (s.flag != 0) return false;
        for (int e = tid; e < D * ng; e += kTrackThreads) {
            const int i = e / ng, c = e - i * ng;
            double r = 0.0;
            for (int j = 0; j < D; ++j) r = r + s.Quu[i * D + j] * s.G[j * ng + c];
            s.M[e] = r + (c == 0 ? s.Qu[i] : s.Qux[i * n + c - 1]);
        }
        __syncthreads();
        for (int e = tid; e < n * n; e += kTrackThreads) {
            const int r = e / n, c = e - r * n;
            double x1 = 0.0, x2 = 0.0;
            for (int i = 0; i < D; ++i) x1 = x1 + s.G[i * ng + 1 + r] * s.M[i * ng + 1 + c];
            for (int i = 0; i < D; ++i) x2 = x2 + s.Qux[i * n + r] * s.G[i * ng + 1 + c];
            s.Qxx[e] = (s.Qxx[e] + x1) + x2;
        }
        if (tid < n) {
            double x1 = 0.0, x2 = 0.0;
            for (int i = 0; i < D; ++i) x1 = x1 + s.G[i * ng + 1 + tid] * s.M[i * ng];
            for (int i = 0; i < D; ++i) x2 = x2 + s.Qux[i * n + tid] * s.G[i * ng];
            s.vx[tid] = (s.Qx[tid] + x1) + x2;
        }
        __syncthreads();
        for (int e = tid; e < n * n; e += kTrackThreads) {
            const int r = e / n, c = e - r * n;
            s.V[e] = 0.5 * (s.Qxx[e] + s.Qxx[c * n + r]);
        }
        __syncthreads();
    }
    return true;
}

// what lane i needs of step t in the forward pass
template <int DC>
struct FwdStep {
    double q, v, u;
    float k, Kq[DC], Kv[DC];
};

template <int DC>
__device__ __forceinline__ void load_step(FwdStep<DC>& f, const double* x, const double* u, const float* gains, int t, int i, int D,
                                          bool on) {
    const int n = 2 * D, ng = n + 1;
    const float* g = gains + ((size_t)t * D + i) * ng;
    f.q = on ? x[(size_t)t * n + i] : 0.0;
    f.v = on ? x[(size_t)t * n + D + i] : 0.0;
    f.u = on ? u[(size_t)t * D + i] : 0.0;
    f.k = on ? g[0] : 0.0f;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
        f.Kq[c] = on && c < D ? g[1 + c] : 0.0f;
        f.Kv[c] = on && c < D ? g[1 + D + c] : 0.0f;
    }
}

// THE FORWARD PASS: the candidate xn, un from the trajectory x, u and the gains
template <int DC>
__device__ __forceinline__ void forward_pass(const TrackArgs& a, const double* x, const double* u, const float* gains, double* xn,
                                             double* un) {
    const int D = a.D, T = a.T, n = 2 * D, i = threadIdx.x;
    const bool on = i < D;
    const double dt = (double)a.dt;
    double qn = on ? x[i] : 0.0, vn = on ? x[D + i] : 0.0;
    if (on) {
        xn[i] = qn;
        xn[D + i] = vn;
    }
    FwdStep<DC> cur, nxt;
    load_step<DC>(cur, x, u, gains, 0, i, D, on);
    for (int t = 0; t < T - 1; ++t) {
        load_step<DC>(nxt, x, u, gains, t + 1 < T - 1 ? t + 1 : t, i, D, on);
        const double dq = qn - cur.q, dv = vn - cur.v;
        double acc = cur.u + (double)cur.k;
#pragma unroll
        for (int c = 0; c < DC; ++c)
            if (c < D) acc = acc + (double)cur.Kq[c] * __shfl(dq, c, kTrackThreads);
#pragma unroll
        for (int c = 0; c < DC; ++c)
            if (c < D) acc = acc + (double)cur.Kv[c] * __shfl(dv, c, kTrackThreads);
        const double q1 = qn + dt * vn;
        vn = vn + dt * acc;
        qn = q1;
        if (on) {
            un[(size_t)t * D + i] = acc;
            xn[(size_t)(t + 1) * n + i] = qn;
            xn[(size_t)(t + 1) * n + D + i] = vn;
        }
        cur = nxt;
    }
    __syncthreads();
}

template <int DC>
__global__ __launch_bounds__(kTrackThreads) void k_motion_track(const TrackArgs a) {
    __shared__ TrackLds<DC> s;
    const int D = a.D, T = a.T, n = 2 * D, ng = n + 1, tri = D * (D + 1) / 2, tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const float* path = a.path + row * (size_t)T * 3;
    const float* init = a.init + row * (size_t)T * D;
    const double dt = (double)a.dt;

    load_chain<DC>(a.frames, a.axes, D, s.frames, s.axes, kTrackThreads);
    bool bad = false;
    if (a.limits) {
        for (int i = tid; i < 2 * D; i += kTrackThreads) {
            const float v = a.limits[i];
            s.lim[i] = v;
            bad = bad || !isfinite(v);
        }
    }
    for (int e = tid; e < D * D; e += kTrackThreads) {
        const int i = e / D, j = e - i * D;
        double v = i == j ? (double)a.R : 0.0;
        if (a.effort) {
            double r = 0.0;
            for (int k = 0; k < D; ++k) r = r + (double)a.effort[k * D + i] * (double)a.effort[k * D + j];
            v = (double)a.R * r;
        }
        s.Se[e] = v;
    }
    for (int i = tid; i < 3 * T; i += kTrackThreads) bad = bad || !isfinite(path[i]);
    for (int i = tid; i < T * D; i += kTrackThreads) bad = bad || !isfinite(init[i]);
    const bool bad_row = __any(bad) != 0;
    __syncthreads();

    // the row's workspace (avae_track.h)
    unsigned char* ws = a.workspace + row * a.row_bytes;
    double* xb = reinterpret_cast<double*>(ws);
    double* ub = xb + 2 * (size_t)T * n;
    float* gains = reinterpret_cast<float*>(ub + 2 * (size_t)T * D);
    float* lq = gains + (size_t)T * D * ng;
    float* lqq = lq + (size_t)T * D;
    double *x = xb, *xn = xb + (size_t)T * n, *u = ub, *un = ub + (size_t)T * D;

    double J = 0.0, J0 = 0.0, sq = 0.0;
    int status = 3, iters = 0, acc = 0;
    if (!bad_row) {
        // THE FIRST CONTROLS and their rollout
        if (tid < D) {
            double q = (double)init[tid], v = 0.0, v0 = 0.0;
            x[tid] = q;
            x[D + tid] = v;
            for (int t = 0; t < T - 1; ++t) {
                const double v1 = ((double)init[(size_t)(t + 1) * D + tid] - (double)init[(size_t)t * D + tid]) / dt;
                const double ut = (v1 - v0) / dt;
                v0 = v1;
                u[(size_t)t * D + tid] = ut;
                const double q1 = q + dt * v;
                v = v + dt * ut;
                q = q1;
                x[(size_t)(t + 1) * n + tid] = q;
                x[(size_t)(t + 1) * n + D + tid] = v;
            }
        }
        __syncthreads();
        J = point_pass<DC, true>(a, s, path, x, u, lq, lqq, sq);
        J0 = J;
        status = T == 1 ? 0 : 1;
        double lam = a.lam0;
        while (T > 1 && iters < a.n_iters) {
            ++iters;
            bool accept = false;
            double Jn = 0.0, sqn = 0.0;
            if (backward_pass<DC>(a, s, u, lq, lqq, gains, lam)) {
                forward_pass<DC>(a, x, u, gains, xn, un);
                Jn = point_pass<DC, false>(a, s, path, xn, un, nullptr, nullptr, sqn);
                accept = Jn < J;
            }
            __syncthreads();                                    // (a rejected backward pass leaves readers of the LDS behind it)
            if (accept) {
                double* sw = x; x = xn; xn = sw;
                sw = u; u = un; un = sw;
                const bool conv = J - Jn < a.tol * J;
                J = Jn;
                sq = sqn;
                lam = lam / a.factor > a.lam_min ? lam / a.factor : a.lam_min;
                ++acc;
                if (conv) { status = 0; break; }
                if (iters < a.n_iters) point_pass<DC, true>(a, s, path, x, u, lq, lqq, sqn);
            } else {
                lam = lam * a.factor;
                if (lam > a.lam_max) { status = acc > 0 ? 0 : 2; break; }
            }
        }
    }
    const float nanf_ = __builtin_nanf("");
    for (int i = tid; i < T * D; i += kTrackThreads) {
        const int t = i / D, c = i - t * D;
        a.traj[row * (size_t)T * D + i] = bad_row ? nanf_ : (float)x[(size_t)t * n + c];
    }
    if (a.controls)
        for (int i = tid; i < (T - 1) * D; i += kTrackThreads) a.controls[row * (size_t)(T - 1) * D + i] = bad_row ? nanf_ : (float)u[i];
    if (tid == 0) {
        const double nan = __builtin_nan("");
        if (a.cost0) a.cost0[row] = bad_row ? nan : J0;
        if (a.cost) a.cost[row] = bad_row ? nan : J;
        if (a.rmse) a.rmse[row] = bad_row ? nanf_ : (float)sqrt(sq / (double)T);
        if (a.iterations) a.iterations[row] = iters;
        if (a.accepted) a.accepted[row] = acc;
        if (a.status) a.status[row] = status;
    }
}

}  // namespace

void launch_motion_track(const TrackArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)a.rows), block(kTrackThreads);
    if (a.D <= 4) launch_kernel(k_motion_track<4>, grid, block, 0, s, a);
    else if (a.D <= 8) launch_kernel(k_motion_track<8>, grid, block, 0, s, a);
    else launch_kernel(k_motion_track<16>, grid, block, 0, s, a);
}

}  // namespace avae
