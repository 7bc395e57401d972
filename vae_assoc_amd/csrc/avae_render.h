// Pen-path kinematics and stroke rendering (avae_motion_fk / avae_stroke_render; include/avae.h): the launch
// shapes and the kernel arguments shared by the host (avae_host.hip) and the kernels (avae_render.hip).
//
// k_motion_fk      one thread per (row, t), 256 per workgroup, a workgroup per tile of 256 consecutive points (grid-stride).  The
//                  tile's angles come in through LDS (consecutive lanes load consecutive floats; a point's D angles sit in a row
//                  of odd length D | 1) and its 768 tip coordinates go out the same way; the chain constants (frames, axes: at most
//                  252 floats) sit in LDS and are read as broadcasts.  The tip alone is wanted, so the chain is applied to a
//                  vector from the tip inwards:  v = frame[D].p;  for j = D - 1 .. 0:  w = Rot(axis_j, q_j) v (Rodrigues:
//                  (v c + (a x v) s) + a ((a . v)(1 - c)), a . v = (ax vx + ay vy) + az vz, the cross product two products and
//                  a difference per component),  v = ((R0 wx + R1 wy) + R2 wz) + p  per row of frame[j].  Plain fp32 multiplies
//                  and adds in the order written, no fma; sincosf is the precise one.  LDS 21.0 KiB, 68 VGPRs, no scratch.
// k_stroke_render  one workgroup of 256 threads per row.  In order:
//   1. thread i loads the points t = i, i + 256, i + 512, i + 768 and adds them up in that order from 0; the 256 partial sums go
//      through THE TREE (for s = 128, 64 .. 1: x[i] = x[i] + x[i + s], i < s); mean = sum / T.  A non-finite coordinate anywhere
//      in the row ends it here: every output of the row is NaN, written as such.
//   2. c_t = (fma(u2, dz, fma(u1, dy, u0 * dx)), the same with v), d = p_t - mean; the exact min / max of both coordinates and the
//      height sum  sum_t (fma(n2, pz, fma(n1, py, n0 * px)) - height)^2  (fma chain per thread, t ascending, then THE TREE) share
//      one tree.  lo = min - r, hi = max + r, ctr = (lo + hi) * 0.5, L = max(hi_u - lo_u, hi_v - lo_v), W = (1 + margin) * L,
//      delta = W / (H * ss), u0 = ctr_u - 0.5 * W, v0 = ctr_v + 0.5 * W.
//   3. segment records in LDS: (A, B - A) as one float4 and inv = 1 / |B - A|^2, or 0 where |B - A|^2 < 1e-30 (such a segment is
//      the point A); T = 1 is one such record.
//   4. pixel classification (culling): the squared distance of a pixel's centre to the polyline, two pixels per thread and
//      segment record; a pixel is inked when that is below thr^2, thr = (r + delta / 2 + 0.7072 ss delta) * 1.002.  A pixel whose
//      centre is at least thr from the bounding box of the points skips the segments.  The inked pixels are compacted into a
//      list in pixel order (wave ballots, a prefix over the <= 64 chunk counts; no atomics).
//   5. a thread owns one sub-row (ss samples) of an inked pixel, 256 / ss pixels per pass: per segment  px = u - Ax, py = v - Ay,
//      t = clamp(fma(px, dx, py * dy) * inv, 0, 1), e = (fma(-t, dx, px), fma(-t, dy, py)), d2 = fma(ey, ey, ex * ex), running
//      min; then d = sqrtf(min), cov = clamp(0.5 + (r - d) / delta, 0, 1) (IEEE square root and division).  A sub-row's
//      coverages are added left to right, a pixel's sub-row sums top to bottom, times 1 / ss^2 (exact).  u = fma(b + 0.5, delta,
//      u0), v = fma(-(a + 0.5), delta, v0).
//   6. the image leaves LDS with consecutive lanes on consecutive pixels; img_l2: thread i adds (image - target)^2 of the pixels
//      i, i + 256, ... (fma chain), THE TREE, sqrtf.
//   Culling changes no bit: cov is exactly +0 once d >= r + delta / 2 (r - d <= -delta / 2 survives rounding, so does the
//   quotient <= -0.5, and the clamp selects +0), a sample lies within ss delta / sqrt(2) of its pixel's centre, and the 0.2 %
//   added to thr is more than 10 times the fp32 error of either distance (below 3e-4 delta at the largest H ss = 512): a pixel
//   that is not inked would get +0 from every sample, which is what the image holds from the start.
//   LDS: 28 T + 6 H^2 bytes + 6.8 KiB (14.3 KiB at T = 100, H = 28: the 32 waves of a CU, not LDS, bound its 8 workgroups; 59.0 KiB
//   at T = 1024, H = 64), 39 / 39 / 45 / 49 VGPRs at ss = 1 / 2 / 4 / 8, no scratch.
// Neither kernel uses atomics or scratch memory or reads or writes anything of the handle.  k_stroke_render's device code lives in
// avae_render_dev.h (render_row), which the reverse pass of avae_grad.hip runs too.
#pragma once
#include "avae_latent_common.h"

namespace avae {

constexpr int kRenderThreads = 256;
constexpr int kFkMaxD = 16, kRenderMaxT = 1024, kRenderMaxH = 64, kRenderMaxSs = 8;
constexpr float kRenderMinLen2 = 1e-30f;      // a shorter segment (squared) is a point
constexpr float kRenderHalfDiag = 0.7072f;    // > sqrt(2) / 2
constexpr float kRenderCullSafety = 1.002f;

struct FkArgs {
    const float* traj;            // [rows][T][D]
    const float* frames;          // [D + 1][3][4]
    const float* axes;            // [D][3]
    float* path;                  // [rows][T][3]
    long long points;             // rows * T
    int D;
};

struct RenderArgs {
    const float* path;            // [rows][T][3]
    const float* plane;           // [3][3]: rows u, v, n
    const float* target;          // [rows][H * H] or NULL
    const float* height;          // [rows] or NULL
    float* image;                 // [rows][H * H] or NULL
    float* window;                // [rows][3] or NULL
    float* img_l2;                // [rows] or NULL
    float* height_l2;             // [rows] or NULL
    float half_width, margin;
    int T, H, ss;
};

// dynamic LDS of k_stroke_render in floats: segment records (float4, first: 16-byte aligned), inv, cu, cv, image, the tree's
// five columns, a pass's sub-row sums, the chunk masks (64 x 8 bytes), the chunk bases (65), the inked list (16 bit each)
struct RenderLds { int seg, inv, cu, cv, img, red, rows, mask, base, list, floats; };
__host__ __device__ inline RenderLds render_lds(int T, int H) {
    RenderLds l;
    const int nseg = T > 1 ? T - 1 : 1, npx = H * H;
    l.seg = 0;
    l.inv = l.seg + 4 * nseg;
    l.cu = l.inv + nseg;
    l.cv = l.cu + T;
    l.img = l.cv + T;
    l.red = l.img + npx;
    l.rows = l.red + 5 * kRenderThreads;
    l.mask = (l.rows + kRenderThreads + 1) & ~1;      // 8-byte aligned
    l.base = l.mask + 128;
    l.list = l.base + 66;
    l.floats = l.list + (npx + 1) / 2;
    return l;
}
inline size_t render_lds_bytes(int T, int H) { return (size_t)render_lds(T, H).floats * 4; }

void launch_motion_fk(const FkArgs& a, hipStream_t s);
void launch_stroke_render(const RenderArgs& a, long long rows, hipStream_t s);

}  // namespace avae
