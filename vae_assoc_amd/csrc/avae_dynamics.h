// Joint-space inertia and inverse dynamics of a serial chain (avae_motion_dynamics; include/avae.h): the launch
// shape and the kernel arguments shared by the host (avae_host.hip) and the kernel (avae_dynamics.hip).
//
// The chain is avae_motion_pose's (frames [D + 1][3][4], axes [D][3]); body k is bodies[k] = (m, c[3], Ixx, Ixy, Ixz, Iyy, Iyz, Izz):
// mass, centre of mass and inertia about it of everything that turns with joint k and not with joint k + 1, in the frame THE WALK has
// right behind joint k's own rotation (KinematicChain.bodies).  Plain fp32 multiplies and adds in the order written, no fma; a x b is
// (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), two products and a difference per component.
//
// THE WALK WITH BODIES (one lane per point).  THE WALK of avae_ik.h, joint by joint, with (s, c) = the double-precision sine and cosine
// of the float angle rounded once (walk<DC, true>'s: the bits do not depend on a float math library).  Right behind joint j's
// rotation, with R = R_j^+:
//     r_j[i]    = (R[i][0] c[0] + R[i][1] c[1]) + R[i][2] c[2]                            (the centre of mass from o_j, base frame)
//     A[i][k]   = (R[i][0] I[0][k] + R[i][1] I[1][k]) + R[i][2] I[2][k]                   (I the symmetric 3 x 3 of the six numbers)
//     I_j[i][k] = (A[i][0] R[k][0] + A[i][1] R[k][1]) + A[i][2] R[k][2],  i <= k          (six numbers, used for both triangles)
//   Frame D is not applied: no quantity below needs the tip.
//   avae_walk.h's walk() keeps o_j and z_j but only the last R, so the loop over the joints is written out here around its
//   apply_frame; giving walk() a hook instead moved the register allocation of k_motion_ik and k_motion_track.
//
// THE PASS (recursive Newton-Euler in base-frame coordinates) takes speeds v, accelerations a, a start acceleration g and a flag
// has_v, and gives tau[D].  Outwards, from w = dw = 0 and ao = g, for j = 0 .. D - 1:
//     j > 0:   d = o_j - o_(j-1);   ao = (ao + dw x d) + w x (w x d)                      (has_v false: ao = ao + dw x d)
//     dw = (dw + z_j a_j) + (w x z_j) v_j   with the old w;   w = w + z_j v_j             (has_v false: dw = dw + z_j a_j, w stays 0)
//     ac = (ao + dw x r_j) + w x (w x r_j)                                                (has_v false: ac = ao + dw x r_j)
//     F_j = m_j ac
//     N_j = I_j dw + w x (I_j w),   (I x)[i] = (I[i][0] x0 + I[i][1] x1) + I[i][2] x2     (has_v false: N_j = I_j dw)
//   inwards, for j = D - 1 .. 0:
//     j = D - 1:   n = N_j + r_j x F_j,   f = F_j
//     else:        n = ((N_j + r_j x F_j) + n) + (o_(j+1) - o_j) x f   with the old f;   f = f + F_j
//     tau_j = (z_j[0] n[0] + z_j[1] n[1]) + z_j[2] n[2]
//   With has_v false the terms in w are left out, not multiplied by zero.
//
// THE OUTPUTS of a point, each by a pass of its own, so that none depends on which others are asked for:
//     gravity  = PASS(v = 0, a = 0,   g = -grav, has_v = false)
//     coriolis = PASS(v,     a = 0,   g = 0,     has_v = vel given)
//     torque   = PASS(v,     a,       g = -grav, has_v = vel given)                       (acc not given: a = 0)
//     inertia: for j = 0 .. D - 1:  t = PASS(v = 0, a = e_j, g = 0, has_v = false);  M[i][j] = M[j][i] = t[i] for i <= j
//   -- D unit-acceleration passes, the upper triangle of each column kept and mirrored, so M is symmetric bit for bit.  -grav is
//   formed on the host (a sign flip).  A point with a non-finite angle, speed or acceleration has NaN in every output.
//
// k_motion_dynamics<DC>, DC = 4, 8, 16 for D <= DC (a joint j >= D is skipped by a uniform branch): one lane per (row, t) point, 64 per
// workgroup (one wave), a workgroup per tile of 64 consecutive points (grid-stride).  The chain and body constants sit in LDS and are
// read as broadcasts.  Angles, speeds and accelerations come in one after the other through one LDS tile (rows of odd length D | 1)
// and every pass's tau[D] goes out through the same tile: a gravity / coriolis / torque tile is one contiguous run of 64 D floats; a
// column of M goes out as the row M[j][0 .. j] of each point (runs of j + 1 floats) and its mirror image M[0 .. j][j] (single
// floats, D apart).  What the walk leaves per joint -- o_j, z_j, r_j and I_j, 15 floats -- lives in lane-private LDS columns
// world_s[quantity][joint][lane]: a wave reads and writes 64 consecutive floats, free of bank conflicts, and the walk is one
// runtime loop over the joints (one copy of the double-precision sincos) that reads its angles from the tile.  The passes are one
// runtime loop around one copy of THE PASS, whose loops over the joints are unrolled: F_j and N_j (6 D floats), the speeds and
// the accelerations (2 D) are registers; a compiler barrier per joint keeps the column loads where they are used and not hoisted
// out of the loop over the passes.  DC = 16 takes 65.9 KiB of a CU's 160 KiB of LDS (two workgroups a CU).
//   Resources (the compiler's resource report): VGPRs / AGPRs / LDS bytes / scratch bytes
//       <4> 109 / 0 / 17088 / 0    <8> 149 / 0 / 33872 / 0    <16> 228 / 0 / 67440 / 0
// No atomics, no scratch memory, nothing of the handle read or written.
#pragma once
#include "avae_ik.h"

namespace avae {

constexpr int kDynThreads = 64;
constexpr int kDynBody = 10;      // floats a body
constexpr int kDynWorld = 15;     // floats a joint in the lane's LDS columns: o, z, r (3 each), I (6)

struct DynArgs {
    const float* traj;            // [rows][T][D]
    const float* vel;             // [rows][T][D] or NULL (v = 0)
    const float* acc;             // [rows][T][D] or NULL (a = 0)
    const float* frames;          // [D + 1][3][4]
    const float* axes;            // [D][3]
    const float* bodies;          // [D][10]
    float* inertia;               // [rows][T][D][D] or NULL
    float* gravity;               // [rows][T][D] or NULL
    float* coriolis;              // [rows][T][D] or NULL
    float* torque;                // [rows][T][D] or NULL
    long long points;             // rows * T
    float g[3];                   // -gravity
    int D;
};

void launch_motion_dynamics(const DynArgs& a, hipStream_t s);

}  // namespace avae
