// Device-visible descriptors of avae_complete (gradient latent refinement for partially observed rows), shared by the host
// planner (avae_host.hip) and the kernels (avae_kernels.hip).
//
// A chunk of at most batch_size rows makes n_iters + 1 passes
//   decoders forward (GEMM launches) -> k_complete_out -> decoder input gradients (GEMM launches) -> k_complete_update
// and the passes are replayed from captured graphs, so their kernel arguments never change: what differs from call to call and
// from pass to pass sits in a device-side CompleteCall.  k_complete_begin writes it (by value from its own arguments), and the
// two kernels of a pass count the passes for each other: k_complete_out reads n_upd and sets n_out, k_complete_update reads
// n_out and sets n_upd.  Neither kernel reads a word that its own workgroups write, and launches are stream-ordered.
#pragma once
#include "avae_device.h"

namespace avae {

struct CompleteCall {
    const float* x[kMaxMod];           // the caller's rows of the chunk; NULL: the modality is unobserved on every row
    long long ldx[kMaxMod];
    const unsigned char* obs[kMaxMod]; // element masks, dense [rows][n_input], nonzero = observed; NULL: every element observed
    float* xhat[kMaxMod];              // nullable: decoder outputs at the final z, dense [rows][n_input]
    const float* z0;                   // [rows][n_z] fp32, dense
    float* z_out;                      // [rows][n_z]
    float* obj;                        // nullable: J of pass t at obj[t * obj_ld + row]
    long long obj_ld;
    float* grad;                       // nullable: dJ/dz of pass 0, dense [rows][n_z]
    int rows, n_iters;
    float lr, prior;
    int n_out, n_upd;                  // passes finished by k_complete_out / k_complete_update
};

// What stays the same for every call on a handle: the plan's buffers.  `bucket` = rows of the plan (batch_size).
struct CompleteArgs {
    CompleteCall* call;
    float* z32; float* m; float* v;    // [bucket][n_z] fp32: z and its Adam moments
    float* recon;                      // [bucket][n_mod]: recon_obs of the pass
    void* Z[kMaxMod]; int ldz[kMaxMod];            // decoder inputs, compute dtype
    const float* out32[kMaxMod]; int ld32[kMaxMod]; // decoder outputs of the pass (p or x_hat), fp32
    void* dO[kMaxMod]; int lddo[kMaxMod];          // output layers' activation gradients, compute dtype
    const float* dz[kMaxMod]; int lddz[kMaxMod];   // fp32 dJ_m/dz of every modality
    int n_in[kMaxMod], binary[kMaxMod];
    float w[kMaxMod];
    float beta1, beta2, eps;
    int n_mod, nz, bucket;
};

void launch_complete_begin(int compute_dtype, const CompleteArgs& a, const CompleteCall& call, hipStream_t s);
void launch_complete_out(int compute_dtype, const CompleteArgs& a, hipStream_t s);
void launch_complete_update(int compute_dtype, const CompleteArgs& a, hipStream_t s);

}  // namespace avae
