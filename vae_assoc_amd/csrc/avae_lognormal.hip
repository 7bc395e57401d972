// Sigma-lognormal stroke kernels (avae_lognormal.h, include/avae.h): k_lognormal_eval, k_lognormal_sample,
// k_lognormal_fit.
#include "avae_device.h"
#include "avae_philox.h"
#include "avae_lognormal.h"

namespace avae {

namespace {

// Every operation below is the one avae_lognormal.h writes, in its order: tests/lognormal_reference.py restates them one by one.
#pragma clang fp contract(off)

constexpr float kSqrt2Pi = 2.5066282746f, kInvSqrtPi = 0.5641895835f;

// The four transcendental functions of THE COMPONENT: the double-precision function of the float argument, rounded once.  That is
// the correctly rounded float result (but for double's own last bit), so the bits do not depend on which of the values within
// its ulp a float math library returns -- the Jacobian's conditioning multiplies that choice by z / sigma, up to 30.
__device__ __forceinline__ float ln32(float x) { return (float)log((double)x); }
__device__ __forceinline__ float exp32(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float erf32(float x) { return (float)erf((double)x); }
__device__ __forceinline__ void sincos32(float x, float* sn, float* cs) {
    double s, c;
    sincos((double)x, &s, &c);
    *sn = (float)s;
    *cs = (float)c;
}

// THE COMPONENT at time t; with JAC also d(vx, vy) / d(the six parameters)
template <bool JAC>
__device__ __forceinline__ void component(const float* p, float t, float& vx, float& vy, float* jx, float* jy) {
    const float D = p[0], t0 = p[1], mu = p[2], sigma = p[3], ths = p[4], the = p[5];
    const float tau = t - t0;
    const float sg = fmaxf(sigma, 1e-6f);
    const bool on = tau >= 1e-6f;
    const float tc = fmaxf(tau, 1e-6f);
    const float z = (ln32(tc) - mu) / sg;
    const float u = on ? exp32(-(z * z) * 0.5f) / ((sg * kSqrt2Pi) * (tc + 1e-5f)) : 0.0f;
    const float amp = D * u;
    const float a = fabsf(amp);
    const float E = erf32(z);
    const float q = the - ths;
    const float phi = ths + (q * 0.5f) * (1.0f + E);
    float sn, cs;
    sincos32(phi, &sn, &cs);
    vx = a * cs;
    vy = a * sn;
    if (JAC) {
        const float s = amp > 0.0f ? 1.0f : (amp < 0.0f ? -1.0f : 0.0f);
        const float sa = s * amp;
        const float K = -(q * kInvSqrtPi) * exp32(-(z * z));
        const float H = 0.5f * (1.0f + E);
        const float da[6] = {s * u, sa * (1.0f / (tc + 1e-5f) + z / (sg * tc)), (sa * z) / sg, (sa * (z * z - 1.0f)) / sg, 0.0f, 0.0f};
        const float dphi[6] = {0.0f, K * (on ? 1.0f / (sg * tc) : 0.0f), K * (1.0f / sg), K * (z / sg), 1.0f - H, H};
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            jx[j] = da[j] * cs - (a * sn) * dphi[j];
            jy[j] = da[j] * sn + (a * cs) * dphi[j];
        }
    }
}

// THE SCAN over the wave's 64 lanes (inclusive)
__device__ __forceinline__ float wave_scan(float x, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float y = __shfl_up(x, off, 64);
        x = lane >= off ? x + y : x;
    }
    return x;
}

// THE BUTTERFLY: every lane gets the sum
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = x + __shfl_xor(x, off, 64);
    return x;
}

__device__ __forceinline__ bool row_is_bad(const float* p_s, int count, float x0, float y0, int lane) {
    bool bad = !(isfinite(x0) && isfinite(y0));
    for (int i = lane; i < 6 * count; i += kLnThreads) bad = bad || !isfinite(p_s[i]);
    return __any(bad) != 0;
}

// one wave evaluates a stroke from the components in LDS: out[k] (and vel[k]) for k < T
__device__ __forceinline__ void wave_stroke(const float* p_s, int count, float x0, float y0, float dt, int T, bool bad,
                                            float* out, float* vel, int lane) {
    const float nan = __builtin_nanf("");
    float cx = 0.0f, cy = 0.0f;
    for (int k0 = 0; k0 < T; k0 += kLnThreads) {
        const int k = k0 + lane;
        float vx = 0.0f, vy = 0.0f;
        if (k < T) {
            const float t = (float)k * dt;
            for (int c = 0; c < count; ++c) {
                float ax, ay;
                component<false>(p_s + 6 * c, t, ax, ay, nullptr, nullptr);
                vx = vx + ax;
                vy = vy + ay;
            }
        }
        const float sx = cx + wave_scan(vx, lane), sy = cy + wave_scan(vy, lane);
        cx = __shfl(sx, 63, 64);
        cy = __shfl(sy, 63, 64);
        if (k < T) {
            out[2 * k] = bad ? nan : x0 + dt * sx;
            out[2 * k + 1] = bad ? nan : y0 + dt * sy;
            if (vel) {
                vel[2 * k] = bad ? nan : vx;
                vel[2 * k + 1] = bad ? nan : vy;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ eval
__global__ __launch_bounds__(kLnThreads) void k_lognormal_eval(const LnEvalArgs a) {
    __shared__ float p_s[kLnMaxC * 6];
    const int lane = threadIdx.x;
    const size_t row = blockIdx.x;
    int count = a.count ? a.count[row] : a.C;
    count = count < 0 ? 0 : (count > a.C ? a.C : count);
    for (int i = lane; i < 6 * count; i += kLnThreads) p_s[i] = a.params[row * a.C * 6 + i];
    __syncthreads();
    const float x0 = a.start[2 * row], y0 = a.start[2 * row + 1];
    const bool bad = row_is_bad(p_s, count, x0, y0, lane);
    wave_stroke(p_s, count, x0, y0, a.dt, a.T, bad, a.path + row * a.T * 2, a.velocity ? a.velocity + row * a.T * 2 : nullptr, lane);
}

// ------------------------------------------------------------------------------------------------ sample
__global__ __launch_bounds__(kLnThreads) void k_lognormal_sample(const LnSampleArgs a) {
    __shared__ float p_s[kLnMaxC * 6];
    __shared__ float path_s[kLnMaxT * 2];
    const int lane = threadIdx.x;
    const size_t row = blockIdx.x / (unsigned)a.S;
    const unsigned smp = blockIdx.x - (unsigned)(row * a.S);
    int count = a.count ? a.count[row] : a.C;
    count = count < 0 ? 0 : (count > a.C ? a.C : count);
    if (lane < a.C) {
        float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (lane < count) {
            const float* src = a.params + (row * a.C + lane) * 6;
            unsigned w[4];
            float nrm[4];
            philox4x32_10(a.row0 + (unsigned)row, smp, (unsigned)lane, 0u, (unsigned)a.seed, (unsigned)(a.seed >> 32) ^ kLnSalt, w);
            box_muller4(w, nrm);
            const float n0 = nrm[0] / 3.0f, n1 = nrm[1] / 3.0f, n2 = nrm[2] / 3.0f;
            const float D = src[0], ths = src[4], the = src[5];
            v[0] = D + (n0 * a.amplitude) * D;
            v[1] = src[1]; v[2] = src[2]; v[3] = src[3];
            v[4] = ths + n1 * a.angle;
            v[5] = (the + n1 * a.angle) + (n2 * a.straightness) * (the - ths);
#pragma unroll
            for (int j = 0; j < 6; ++j) p_s[6 * lane + j] = v[j];
        }
        if (a.perturbed) {
            float* dst = a.perturbed + ((row * a.S + smp) * a.C + lane) * 6;
#pragma unroll
            for (int j = 0; j < 6; ++j) dst[j] = v[j];
        }
    }
    __syncthreads();
    const float x0 = a.start[2 * row], y0 = a.start[2 * row + 1];
    const bool bad = row_is_bad(p_s, count, x0, y0, lane);
    float* out = a.strokes + (row * a.S + smp) * (size_t)a.T * 2;
    if (!a.shift_mean) {
        wave_stroke(p_s, count, x0, y0, a.dt, a.T, bad, out, nullptr, lane);
        return;
    }
    wave_stroke(p_s, count, x0, y0, a.dt, a.T, bad, path_s, nullptr, lane);
    __syncthreads();
    float sx = 0.0f, sy = 0.0f;
    for (int k = lane; k < a.T; k += kLnThreads) {
        sx = sx + path_s[2 * k];
        sy = sy + path_s[2 * k + 1];
    }
    const float mx = wave_sum(sx) / (float)a.T, my = wave_sum(sy) / (float)a.T;
    for (int k = lane; k < a.T; k += kLnThreads) {
        out[2 * k] = path_s[2 * k] - mx;
        out[2 * k + 1] = path_s[2 * k + 1] - my;
    }
}

// ------------------------------------------------------------------------------------------------ fit
template <int CC>
struct FitLds {
    static constexpr int P = 6 * CC;
    static constexpr int TT = CC == 16 ? 8 : kLnFitThreads / CC;
    double M[P * (P + 1) / 2];
    double g[P], d[P];
    double e[TT * 4];
    double loss, pivot;
    float J[TT * 4 * P];
    float vc[TT * CC * 2];
    float p[P], cand[P];
    int flag;
    unsigned char free_mask[P];
};

__device__ __forceinline__ void tri_ij(int e, int& i, int& j) {
    i = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
    while (i * (i + 1) / 2 > e) --i;
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    j = e - i * (i + 1) / 2;
}

// A PASS of avae_lognormal.h at the parameters q (in LDS): the loss; with JAC also M = J^T W J and g = J^T W e into s.M, s.g
template <int CC, bool JAC>
__device__ __forceinline__ double fit_pass(const LnFitArgs& a, FitLds<CC>& s, const float* q, int count, const float* tgt,
                                           float x0, float y0) {
    constexpr int P = FitLds<CC>::P, TT = FitLds<CC>::TT;
    const int tid = threadIdx.x, T = a.T, Pn = 6 * count, ntri = Pn * (Pn + 1) / 2;
    if (JAC) {
        for (int e = tid; e < ntri; e += kLnFitThreads) s.M[e] = 0.0;
        if (tid < Pn) s.g[tid] = 0.0;
    }
    if (tid == 0) s.loss = 0.0;
    const int tt_a = tid / CC, c_a = tid - tt_a * CC;
    const int vt = tid - 2 * Pn;                      // 0, 1: the value threads (x, y)
    float run = 0.0f;                                 // a column's running sum, carried over the tiles
    float prev = vt == 0 ? x0 : y0;                   // the value threads: the target point before
    for (int k0 = 0; k0 < T; k0 += TT) {
        const int nt = T - k0 < TT ? T - k0 : TT;
        // A
        if (tt_a < nt && c_a < count) {
            float vx, vy, jx[6], jy[6];
            component<JAC>(q + 6 * c_a, (float)(k0 + tt_a) * a.dt, vx, vy, jx, jy);
            s.vc[(tt_a * CC + c_a) * 2] = vx;
            s.vc[(tt_a * CC + c_a) * 2 + 1] = vy;
            if (JAC) {
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    s.J[(tt_a * 4 + 2) * P + 6 * c_a + j] = jx[j];
                    s.J[(tt_a * 4 + 3) * P + 6 * c_a + j] = jy[j];
                }
            }
        }
        __syncthreads();
        // B
        if (JAC && tid < 2 * Pn) {
            const int i = tid >> 1, xy = tid & 1;
            for (int tt = 0; tt < nt; ++tt) {
                run = run + s.J[(tt * 4 + 2 + xy) * P + i];
                s.J[(tt * 4 + xy) * P + i] = a.dt * run;
            }
        } else if (vt == 0 || vt == 1) {
            for (int tt = 0; tt < nt; ++tt) {
                float v = 0.0f;
                for (int c = 0; c < count; ++c) v = v + s.vc[(tt * CC + c) * 2 + vt];
                run = run + v;
                const float pos = (vt == 0 ? x0 : y0) + a.dt * run;
                const float P_k = tgt[2 * (k0 + tt) + vt];
                const float V_k = (P_k - prev) / a.dt;
                prev = P_k;
                s.e[tt * 4 + vt] = (double)pos - (double)P_k;
                s.e[tt * 4 + 2 + vt] = (double)v - (double)V_k;
            }
        }
        __syncthreads();
        // C
        const int n_c = JAC ? 1 + Pn + ntri : 1;
        for (int e = tid; e < n_c; e += kLnFitThreads) {
            if (e == 0) {
                double L = s.loss;
                for (int r = 0; r < nt * 4; ++r) {
                    const double w = (r & 2) ? a.wv : a.wp, er = s.e[r];
                    L = L + (w * er) * er;
                }
                s.loss = L;
            } else if (e <= Pn) {
                const int i = e - 1;
                double acc = s.g[i];
                for (int r = 0; r < nt * 4; ++r) {
                    const double w = (r & 2) ? a.wv : a.wp;
                    acc = acc + (w * (double)s.J[r * P + i]) * s.e[r];
                }
                s.g[i] = acc;
            } else {
                int i, j;
                tri_ij(e - 1 - Pn, i, j);
                double acc = s.M[e - 1 - Pn];
                for (int r = 0; r < nt * 4; ++r) {
                    const double w = (r & 2) ? a.wv : a.wp;
                    acc = acc + (w * (double)s.J[r * P + i]) * (double)s.J[r * P + j];
                }
                s.M[e - 1 - Pn] = acc;
            }
        }
        __syncthreads();
    }
    const double L = s.loss;
    __syncthreads();
    return L;
}

template <int CC>
__global__ __launch_bounds__(kLnFitThreads) void k_lognormal_fit(const LnFitArgs a) {
    __shared__ FitLds<CC> s;
    const int tid = threadIdx.x, C = a.C, T = a.T;
    const size_t row = blockIdx.x;
    int count = a.count ? a.count[row] : C;
    count = count < 0 ? 0 : (count > C ? C : count);
    const int Pn = 6 * count, ntri = Pn * (Pn + 1) / 2;
    const float* tgt = a.target + row * (size_t)T * 2;
    const float x0 = a.start[2 * row], y0 = a.start[2 * row + 1];

    if (tid == 0) s.flag = 0;
    __syncthreads();
    bool bad = !(isfinite(x0) && isfinite(y0));
    for (int i = tid; i < 2 * T; i += kLnFitThreads) bad = bad || !isfinite(tgt[i]);
    if (tid < Pn) {
        const float v = a.init[row * C * 6 + tid];
        s.p[tid] = v;
        bad = bad || !isfinite(v);
        s.free_mask[tid] = !a.free_mask ? 1 : (a.free_per_row ? a.free_mask[row * C * 6 + tid] : a.free_mask[tid % 6]);
    }
    if (bad) s.flag = 1;
    __syncthreads();
    const bool bad_row = s.flag != 0;
    __syncthreads();

    double L = 0.0, L0 = 0.0, lam = 1e-3;
    int status = 3, iters = 0, acc = 0, rejects = 0;
    if (!bad_row) {
        L = fit_pass<CC, false>(a, s, s.p, count, tgt, x0, y0);
        L0 = L;
        status = count == 0 ? 0 : 1;
        while (count > 0 && iters < a.n_iters) {
            fit_pass<CC, true>(a, s, s.p, count, tgt, x0, y0);
            ++iters;
            // the mask, the damping
            for (int e = tid; e < ntri; e += kLnFitThreads) {
                int i, j;
                tri_ij(e, i, j);
                if (!(s.free_mask[i] && s.free_mask[j])) s.M[e] = i == j ? 1.0 : 0.0;
            }
            if (tid == 0) s.flag = 0;
            __syncthreads();
            if (tid < Pn) {
                const bool fr = s.free_mask[tid] != 0;
                s.d[tid] = fr ? s.M[tid * (tid + 1) / 2 + tid] : 0.0;
                if (!fr) s.g[tid] = 0.0;
            }
            __syncthreads();
            double md = 0.0;
            for (int i = 0; i < Pn; ++i) md = s.d[i] > md ? s.d[i] : md;
            if (tid < Pn && s.free_mask[tid]) s.M[tid * (tid + 1) / 2 + tid] += lam * s.d[tid] + 1e-12 * (md + 1.0);
            __syncthreads();
            // Cholesky, in place
            bool ok = true;
            for (int j = 0; j < Pn; ++j) {
                const int jj = j * (j + 1) / 2;
                if (tid == 0) {
                    double v = s.M[jj + j];
                    for (int k = 0; k < j; ++k) v = v - s.M[jj + k] * s.M[jj + k];
                    s.pivot = v;
                    s.M[jj + j] = sqrt(v);
                }
                __syncthreads();
                if (!(s.pivot > 0.0)) { ok = false; break; }
                const double djj = s.M[jj + j];
                for (int i = j + 1 + tid; i < Pn; i += kLnFitThreads) {
                    const int ii = i * (i + 1) / 2;
                    double v = s.M[ii + j];
                    for (int k = 0; k < j; ++k) v = v - s.M[ii + k] * s.M[jj + k];
                    s.M[ii + j] = v / djj;
                }
                __syncthreads();
            }
            __syncthreads();                                    // (a break leaves the readers of s.pivot behind it)
            if (ok) {
                for (int j = 0; j < Pn; ++j) {
                    const int jj = j * (j + 1) / 2;
                    if (tid == 0) s.g[j] = s.g[j] / s.M[jj + j];
                    __syncthreads();
                    const double yj = s.g[j];
                    for (int i = j + 1 + tid; i < Pn; i += kLnFitThreads) s.g[i] = s.g[i] - s.M[i * (i + 1) / 2 + j] * yj;
                    __syncthreads();
                }
                for (int j = Pn - 1; j >= 0; --j) {
                    const int jj = j * (j + 1) / 2;
                    if (tid == 0) s.g[j] = s.g[j] / s.M[jj + j];
                    __syncthreads();
                    const double xj = s.g[j];
                    for (int i = tid; i < j; i += kLnFitThreads) s.g[i] = s.g[i] - s.M[jj + i] * xj;
                    __syncthreads();
                }
                if (tid < Pn) {
                    const double x = s.g[tid];
                    float v = s.p[tid];
                    if (s.free_mask[tid]) {
                        if (!isfinite(x)) s.flag = 1;
                        const int j = tid % 6;
                        v = (float)((double)v - x);
                        if (j == 3) v = fminf(fmaxf(v, 1e-3f), 3.0f);
                        if (a.lo) v = fmaxf(v, a.lo[j]);
                        if (a.hi) v = fminf(v, a.hi[j]);
                    }
                    s.cand[tid] = v;
                }
                __syncthreads();
                ok = s.flag == 0;
            }
            bool accept = false;
            double Ln = 0.0;
            if (ok) {
                Ln = fit_pass<CC, false>(a, s, s.cand, count, tgt, x0, y0);
                accept = Ln < L;
            }
            if (accept) {
                if (tid < Pn) s.p[tid] = s.cand[tid];
                __syncthreads();
                const bool conv = L - Ln < a.tol * L;
                L = Ln;
                lam = lam / 3.0 > 1e-9 ? lam / 3.0 : 1e-9;
                ++acc;
                rejects = 0;
                if (conv) { status = 0; break; }
            } else {
                lam = 4.0 * lam < 1e9 ? 4.0 * lam : 1e9;
                if (++rejects == 8) { status = acc > 0 ? 0 : 2; break; }
            }
        }
    }
    const float nanf_ = __builtin_nanf("");
    for (int i = tid; i < 6 * C; i += kLnFitThreads) a.params[row * C * 6 + i] = bad_row ? nanf_ : (i < Pn ? s.p[i] : 0.0f);
    if (tid == 0) {
        const double nan = __builtin_nan("");
        if (a.loss0) a.loss0[row] = bad_row ? nan : L0;
        if (a.loss) a.loss[row] = bad_row ? nan : L;
        if (a.iterations) a.iterations[row] = iters;
        if (a.accepted) a.accepted[row] = acc;
        if (a.status) a.status[row] = status;
    }
}

}  // namespace

void launch_lognormal_eval(const LnEvalArgs& a, hipStream_t s) {
    launch_kernel(k_lognormal_eval, dim3((unsigned)a.rows), dim3(kLnThreads), 0, s, a);
}

void launch_lognormal_sample(const LnSampleArgs& a, hipStream_t s) {
    launch_kernel(k_lognormal_sample, dim3((unsigned)((long long)a.rows * a.S)), dim3(kLnThreads), 0, s, a);
}

void launch_lognormal_fit(const LnFitArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)a.rows), block(kLnFitThreads);
    if (a.C <= 4) launch_kernel(k_lognormal_fit<4>, grid, block, 0, s, a);
    else if (a.C <= 8) launch_kernel(k_lognormal_fit<8>, grid, block, 0, s, a);
    else launch_kernel(k_lognormal_fit<16>, grid, block, 0, s, a);
}

}  // namespace avae
