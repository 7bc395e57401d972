/*
 * avae.h -- C ABI of libavae: the MI355X (gfx950) associative-VAE training path.
 *
 * This is the drop-in boundary of the repository.  The reference (navigator8972/vae_assoc) has
 * no FFI of its own: its boundary is the Python class AssocVariationalAutoEncoder whose methods
 * each end in one TensorFlow `sess.run` (reference vae_assoc.py:383,389,399-402,417-418,423-424).
 * Every entry point below replaces one of those `sess.run` calls (cited per function); the
 * Python class in vae_assoc_amd/vae_assoc.py keeps the reference's method surface and calls
 * these through ctypes.
 *
 * Conventions
 *  - plain C types only; device pointers are raw `float*` into HBM owned by the caller
 *    (PyTorch-ROCm tensors are used purely as containers on the Python side);
 *  - every function returns 0 on success, nonzero on failure; the message is available from
 *    avae_last_error(); no C++ exception crosses the ABI;
 *  - one handle = one model replica on one GPU; calls on one handle serialise on an internal
 *    mutex (the reference's callers use the session from a worker thread and the GUI thread,
 *    baxter_vae_assoc_writer.py:651-673); different handles are independent;
 *  - `stream` is a hipStream_t passed as void* (NULL = the HIP null stream).  Work is
 *    enqueued asynchronously; a call only synchronises when it has to hand a host value back
 *    (a non-NULL `cost_host`, get/set of parameters, save/load);
 *  - matrices are row-major; an input batch of modality m is [rows, n_input_m] float32 with a
 *    row stride (leading dimension, in floats) given by `x_ld[m]` (NULL = dense, ld = n_input).
 *
 * Flat parameter order (avae_get_params / avae_set_params / avae_get_grads / Adam state) is the
 * reference's variable-creation order, per modality (vae_assoc.py:185-215,257-300):
 *   enc W1[n_in,H1] b1 W2[H1,H2] b2 ... Wmu[HL,n_z] bmu Wsig[HL,n_z] bsig
 *   dec V1[n_z,H1] c1 V2[H1,H2] c2 ... Vout[HL,n_in] cout         each W row-major [in,out].
 */
#ifndef AVAE_H_
#define AVAE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVAE_ABI_VERSION 4
#define AVAE_MAX_MODALITIES 4
#define AVAE_MAX_HIDDEN 8

/* hidden-layer transfer function: reference `transfer_fct` (vae_assoc.py:26,48,502) */
enum { AVAE_ACT_IDENTITY = 0, AVAE_ACT_RELU = 1, AVAE_ACT_SOFTPLUS = 2, AVAE_ACT_SIGMOID = 3, AVAE_ACT_TANH = 4 };
/* arithmetic type of the GEMM operands (accumulation, losses, latent maths and Adam are fp32) */
enum { AVAE_F32 = 0, AVAE_BF16 = 1 };
/* who runs the gradient all-reduce (avae_config.use_comm) */
enum { AVAE_COMM_NONE = 0, AVAE_COMM_RCCL = 1, AVAE_COMM_IPC = 2 };
#define AVAE_IPC_HANDLE_BYTES 128
#define AVAE_MAX_WORLD 8

typedef struct avae_modality {
    int32_t n_input;                    /* reference network_architecture["n_input"] */
    int32_t n_hidden_layers;            /* 2 in the reference (n_hidden_recog_1/2)   */
    int32_t n_hidden[AVAE_MAX_HIDDEN];  /* encoder widths; the MLP decoder reuses them (vae_assoc.py:257,280,293) */
    int32_t binary;                     /* 1: Bernoulli recon + sigmoid output (:321-324,:293-297); 0: Gaussian (:327-328,:299-303) */
    float weight;                       /* reference `weights[m]` (:319,:340) */
    int32_t hidden_conv;                /* 1: conv encoder / deconv decoder branch (vae_assoc.py:169-210,249-291; deconv.py).
                                           Needs binary=1 and n_input=784 (the branch is hard-wired to 28x28 images);
                                           n_hidden[0..1] = n_hidden_recog_1/2 (conv depths), conv_gener = n_hidden_gener_1/2 */
    int32_t conv_gener[2];
    int32_t reserved;
} avae_modality;

typedef struct avae_config {
    int32_t abi_version;                /* AVAE_ABI_VERSION */
    int32_t n_modalities;
    avae_modality mod[AVAE_MAX_MODALITIES];
    int32_t n_z;                        /* taken from modality 0 in the reference (:89) */
    int32_t batch_size;                 /* rows per train/eval step on THIS replica (reference batch_size, :27,:90) */
    int32_t batch_global;               /* divisor of the mean terms; 0 -> batch_size.  world_size*batch_size under data parallelism */
    int32_t row_offset;                 /* global row index of local row 0 (rank*batch_size): keys the internal eps generator */
    int32_t activation;                 /* AVAE_ACT_* */
    int32_t compute_dtype;              /* AVAE_F32 | AVAE_BF16 */
    int32_t device;                     /* HIP device ordinal */
    int32_t use_graph;                  /* 1: replay the step as a captured hipGraph */
    float assoc_lambda;                 /* reference assoc_lambda (:29,:369) */
    float learning_rate;                /* reference learning_rate (:50,:374) */
    float beta1, beta2, adam_eps;       /* TF-1 AdamOptimizer defaults 0.9 / 0.999 / 1e-8 when all three are 0 */
    uint64_t seed;                      /* Philox key of the internal eps generator */
    void* workspace;                    /* optional caller-owned device memory (>= avae_workspace_bytes); NULL -> hipMalloc */
    size_t workspace_bytes;
    /* Library-owned gradient collective (the reference is single-process, vae_assoc.py:66).
     * use_comm = AVAE_COMM_RCCL: avae_create builds an RCCL communicator of world_size ranks from nccl_id (the 128 bytes of an
     *   ncclUniqueId made by avae_comm_unique_id on rank 0 and handed to every rank by whatever bootstrap the host has --
     *   torch.distributed here); the collective is ncclAllReduce on the library's comm stream.
     * use_comm = AVAE_COMM_IPC: the library's own one-shot all-reduce over hipIpc peers (push reduce-scatter + push all-gather,
     *   every xGMI link at once).  avae_create allocates the replica's exchange block; the host hands every
     *   rank's avae_comm_ipc_handle bytes round and calls avae_comm_ipc_attach before the first step.
     * Either way avae_train_step(s) run backward -> all-reduce -> Adam per bucket on the library's own streams, the decoder-side
     * bucket's all-reduce overlapping the encoder's backward pass, sixteen steps per captured hipGraph.
     * use_comm = AVAE_COMM_NONE: a host that owns the collective drives the same buckets through avae_stage_batches /
     * avae_dp_backward / avae_dp_apply.  batch_global / row_offset above stay the caller's to set (world_size*batch_size,
     * rank*batch_size). */
    int32_t use_comm;                   /* AVAE_COMM_* */
    int32_t world_size;
    int32_t rank;
    int32_t comm_buckets;               /* 0 or 2: two buckets (decoder side first); 1: ONE all-reduce of the whole gradient buffer */
    uint8_t nccl_id[128];
    int32_t wire_dtype;                 /* AVAE_F32 (default) | AVAE_BF16: gradient element type on the wire; the cost slot is always fp32 */
    int32_t reserved2[3];
} avae_config;

typedef struct avae_handle avae_handle;

/* Size of the single device allocation a replica needs (parameters, Adam state, compute-dtype
 * shadows, activations, gradients).  Lets the caller allocate it as a torch tensor. */
int avae_workspace_bytes(const avae_config* cfg, size_t* bytes);

/* Replaces AssocVariationalAutoEncoder.__init__ graph/session construction (vae_assoc.py:26-71).
 * Parameters start at zero: call avae_set_params (weights are injected explicitly because the
 * TF RNG stream of xavier_init, :11-18, cannot be reproduced). */
int avae_create(const avae_config* cfg, avae_handle** out);
void avae_destroy(avae_handle* h);
/* h may be NULL: returns the message of the last failed avae_create on this thread. */
const char* avae_last_error(const avae_handle* h);

int avae_param_count(const avae_handle* h, size_t* n);
int avae_get_params(avae_handle* h, float* host_dst);         /* flat order above, host memory */
int avae_set_params(avae_handle* h, const float* host_src);
/* Gradient of the last applied step, flat order (parity tests).  Inside a run (avae_train_steps) the small nets' fused step stores
 * the gradient only on the last step of each replayed graph -- the earlier ones would be overwritten before the host could ask --
 * so what this returns is unchanged: the last step's. */
int avae_get_grads(avae_handle* h, float* host_dst);
/* Adam slots + step counter: what tf.train.Saver checkpoints besides the weights (vae_assoc.py:70,427-463). */
int avae_get_opt_state(avae_handle* h, float* host_m, float* host_v, int64_t* step);
int avae_set_opt_state(avae_handle* h, const float* host_m, const float* host_v, int64_t step);

/* partial_fit (vae_assoc.py:378-386): one sess.run((optimizer, cost)).
 *   x_dev[m]  device [batch_size, n_input_m] float32, row stride x_ld[m]
 *   eps_dev   device [batch_size, n_z] float32 shared by all modalities (:90), or NULL ->
 *             internal Philox4x32-10 normals keyed by (seed, step, global row)
 *   cost_host NULL -> fully asynchronous; else receives the cost of this step's forward pass
 *             (pre-update weights, as in the reference) after a stream synchronise. */
int avae_train_step(avae_handle* h, const float* const* x_dev, const int32_t* x_ld,
                    const float* eps_dev, float* cost_host, void* stream);
/* The inner batch loop of train() (vae_assoc.py:541-550 over DataSet.next_batch's consecutive slices,
 * dataset.py:22-43) as ONE submission: exactly n_steps successive avae_train_step calls, step i on rows
 * [i*batch_size, (i+1)*batch_size) of every x_dev[m] (row stride x_ld[m]) and of eps_dev (dense [.., n_z];
 * NULL -> internal generator).  Steps are replayed sixteen (then four) to a hipGraph whose first kernel stages
 * all of the replay's batches at once, so the host is out of the loop and the replay boundary and the staging
 * launch are paid once per sixteen steps.  cost_host (optional) receives the LAST step's cost; every step's
 * cost is in avae_cost_history. */
int avae_train_steps(avae_handle* h, int32_t n_steps, const float* const* x_dev, const int32_t* x_ld,
                     const float* eps_dev, float* cost_host, void* stream);
/* ---- the data-parallel seam (the reference has none: one tf.InteractiveSession, vae_assoc.py:66).  The gradient buffer is ONE
 * device array of avae_grad_buffer's n_floats: the local gradient in the master layout (encoder sides of every modality, then
 * decoder sides, pads zero) with the local cost in its last float.  It is cut into buckets of ONE contiguous range each:
 * bucket 0 = decoder sides + the cost slot, bucket 1 = encoder sides; comm_buckets = 1 and models with a conv modality have the
 * single bucket 0 = the whole buffer.  avae_dp_plan is host-only (no GPU needed): offs/counts hold n_buckets entries.
 * Host-owned collective:  avae_stage_batches(n) ; per step j:  avae_dp_backward(j, 0) -> SUM-all-reduce bucket 0's range ->
 * avae_dp_backward(j, 1) -> all-reduce bucket 1's range -> avae_dp_apply(0) -> avae_dp_apply(1). */
int avae_stage_batches(avae_handle* h, int32_t n_steps, const float* const* x_dev, const int32_t* x_ld,
                       const float* eps_dev, void* stream);
int avae_grad_buffer(avae_handle* h, float** dev_ptr, size_t* n_floats);
int avae_dp_plan(const avae_config* cfg, int32_t* n_buckets, int32_t* n_ranges, int64_t* offs, int64_t* counts);
int avae_dp_backward(avae_handle* h, int32_t j, int32_t bucket, void* stream);
int avae_dp_apply(avae_handle* h, int32_t bucket, float* cost_host, void* stream);
/* With avae_set_grad_clip on, avae_dp_apply(0) first sums the squares of the WHOLE gradient buffer, so in the call order above both
 * all-reduces come before it (as documented: apply follows the last all-reduce); avae_dp_apply(1) reuses those partial sums. */
/* 128 bytes of a fresh ncclUniqueId (rank 0 calls this; every rank passes the same bytes in avae_config.nccl_id). */
int avae_comm_unique_id(void* id128);
/* AVAE_COMM_IPC bring-up: AVAE_IPC_HANDLE_BYTES describing this replica's exchange block (a hipIpcMemHandle_t + its size and
 * rank); the host gathers every rank's bytes IN RANK ORDER and hands all world_size * AVAE_IPC_HANDLE_BYTES to attach, which maps
 * the peers' blocks.  Both are collective in the sense that every rank must call them before any rank trains. */
int avae_comm_ipc_handle(avae_handle* h, void* handle_out);
int avae_comm_ipc_attach(avae_handle* h, const void* handles_by_rank);
/* Costs of the most recent `n` applied steps (oldest first), without having synchronised per step. */
int avae_cost_history(avae_handle* h, int32_t n, float* host_dst, int64_t* last_step);

/* ---- partially paired batches (the reference has none: every row carries every modality, vae_assoc.py:90).
 * present_dev: device uint8 [n_steps*batch_size][n_modalities], row-major, nonzero = row n has modality m (p[n,m]).  With B_g =
 * batch_global (= batch_size on one replica) and recon / latent / assoc exactly avae_score's per-row columns (one eps row for every
 * modality), the masked cost is
 *   cost = sum_m w_m [ (1/B_g) sum_n p[n,m] latent[n,m] + (binary_m ? 1/B_g : 1) sum_n p[n,m] recon[n,m] ]
 *        + assoc_lambda sum_{i<j} sum_n p[n,i] p[n,j] assoc[n,i,j]
 * and the step's gradient is its gradient; Adam is unchanged.
 *  - the divisor stays B_g, not the number of present rows: an all-present mask gives the unmasked step bit for bit and shards stay
 *    additive.  Per-modality means: rescale the weights;
 *  - absent entries are never read into the loss: the staging kernel writes zeros for every absent (row, modality) and the loss and
 *    latent terms of absent entries are SELECTED away (not multiplied by 0) -- NaN / Inf / garbage there changes nothing, and an absent
 *    (row, modality) adds exact zeros to every gradient entry of that modality's encoder and decoder.  A row with nothing present
 *    contributes nothing;
 *  - x_dev[m] == NULL: modality m is absent on every row, whatever its column of present_dev says (never read through);
 *  - eps_dev NULL: the internal generator with the unmasked calls' keys ((seed, step, global row) for training, the eval salt and the
 *    per-call draw counter for evaluation); both calls advance the same step / draw counters as their unmasked twins, so masked and
 *    unmasked calls may be interleaved freely on one handle (one step counter, Adam state and cost history);
 *  - present_dev == NULL is an error (use the unmasked entry points), and so is a data-parallel handle (world_size > 1 or use_comm !=
 *    AVAE_COMM_NONE): these calls run on one replica.
 * The first masked call builds the masked twin of the step (its captured graphs and a presence staging buffer of 16 * batch_size *
 * n_modalities bytes, freed by avae_destroy); avae_workspace_bytes is unchanged.
 * avae_train_steps_masked with n_steps = 1 is the masked partial_fit; for n_steps > 1 it follows avae_train_steps step for step (rows of
 * present_dev as of x_dev), costs in avae_cost_history, avae_get_grads = the last step's gradient.  avae_eval_cost_masked: the masked
 * evaluate_cost (batch_size rows, no update). */
int avae_train_steps_masked(avae_handle* h, int32_t n_steps, const float* const* x_dev, const int32_t* x_ld,
                            const uint8_t* present_dev, const float* eps_dev, float* cost_host, void* stream);
int avae_eval_cost_masked(avae_handle* h, const float* const* x_dev, const int32_t* x_ld,
                          const uint8_t* present_dev, const float* eps_dev, float* cost_host, void* stream);

/* ---- denoising training (the reference has none: vae_assoc.py:90 feeds one placeholder to the encoder and to the loss).  Per
 * modality m a step has a target x_m and an encoder input x~_m: the encoder (and its first layer's weight gradient) reads x~_m, the
 * reconstruction term is charged against x_m, so
 *   cost = loss_terms(forward(x~), x)      and the step's gradient is its gradient; presence masks gate as above; Adam is unchanged.
 * x~_m is, in this order of precedence,
 *  1. in_dev[m], an explicit input: device [rows, n_input_m] float32 with its own row stride in_ld[m] (NULL / 0 = dense), read
 *     exactly as x_dev[m] is (any dword alignment, any column block of a wider matrix);
 *  2. x_m corrupted on the device, when avae_set_corruption set a drop_prob or noise_std for m -- per element, iid:
 *       x~ = dropped ? drop_value_m : (noise_std_m > 0 ? x + noise_std_m * n : x),   dropped ~ Bernoulli(drop_prob_m),  n ~ N(0,1)
 *     the drop is a select: a NaN in a dropped element of x does not reach x~ (it still reaches the target, as ever);
 *  3. x_m itself: staging then writes the bits it always wrote.
 * The corruption stream is Philox4x32-10 under the handle's seed, like the eps stream but under salts of its own.  With R the global
 * row (row_offset + local row), q the column quad (column / 4), t the step the batch belongs to (the device step counter + the
 * batch's index in the submission), SALT_DROP = 0x64726f70, SALT_NOISE = 0x6e6f6973:
 *   w = philox(counter = (R, q, t_lo, t_hi ^ (SALT + m)), key = (seed_lo, seed_hi))
 *   drop : element e of the quad is dropped iff (w[e] >> 8) < floor(drop_prob_m * 2^24)        (the product taken in double)
 *   noise: n[0..3] = the Box-Muller pairs of w, formed exactly as the internal eps is
 * so x~ of step t is the same whether the step runs alone or inside a 16- or 4-step replay, masked or not, on one replica or as the
 * shard [row_offset, row_offset + batch_size) of a global batch, and after avae_load / avae_set_opt_state restored the step
 * counter.  Every rank of a data-parallel run must share the seed, as it must for eps.  A stream is drawn only for a modality whose
 * parameter is nonzero.
 * avae_set_corruption: NULL or all zero = off.  Errors (the message names the field): drop_prob outside [0, 1), a negative or
 * non-finite noise_std, a non-finite drop_value.  The setting is handle state, set under the handle's mutex; it is not part of
 * avae_save / avae_load, and work already enqueued keeps the setting it was enqueued with.  Once set, EVERY training call corrupts:
 * avae_train_step, avae_train_steps, avae_train_steps_masked, avae_stage_batches and the library-owned data-parallel pipeline are
 * the _in calls below with in_dev NULL.  Evaluation never corrupts: avae_eval_cost, avae_eval_cost_masked and every inference call
 * are bit for bit what they are without it, and avae_eval_cost_in uses explicit inputs only (the objective on given corrupted
 * inputs).
 * The _in calls: in_dev NULL, or in_dev[m] NULL = no explicit input for m; present_dev NULL = unmasked, else the masked twin (an
 * absent (row, m) reads neither x nor in; a data-parallel handle is refused as avae_train_steps_masked refuses it).  Errors:
 * in_ld[m] < n_input_m; in_dev[m] set while x_dev[m] is NULL.  With every optional argument NULL and no corruption set they are
 * bitwise avae_train_steps / avae_eval_cost / avae_stage_batches. */
typedef struct avae_corruption {
    float drop_prob[AVAE_MAX_MODALITIES];   /* in [0, 1) */
    float drop_value[AVAE_MAX_MODALITIES];  /* finite; 0 = erased ink */
    float noise_std[AVAE_MAX_MODALITIES];   /* >= 0 */
} avae_corruption;
int avae_set_corruption(avae_handle* h, const avae_corruption* corruption);
int avae_train_steps_in(avae_handle* h, int32_t n_steps, const float* const* x_dev, const int32_t* x_ld,
                        const float* const* in_dev, const int32_t* in_ld, const uint8_t* present_dev,
                        const float* eps_dev, float* cost_host, void* stream);
int avae_eval_cost_in(avae_handle* h, const float* const* x_dev, const int32_t* x_ld,
                      const float* const* in_dev, const int32_t* in_ld, const uint8_t* present_dev,
                      const float* eps_dev, float* cost_host, void* stream);
int avae_stage_batches_in(avae_handle* h, int32_t n_steps, const float* const* x_dev, const int32_t* x_ld,
                          const float* const* in_dev, const int32_t* in_ld, const float* eps_dev, void* stream);

/* ---- global-norm gradient clipping and non-finite step skipping (the reference has neither: a bare tf.train.AdamOptimizer,
 * vae_assoc.py:373-374; what a TF-1 caller writes as tf.clip_by_global_norm in front of apply_gradients).  Per step, with g the
 * step's gradient over the whole model (one replica: the local gradient; data parallel: the all-reduced one; masked and denoising
 * steps included; the cost slot excluded):
 *   s    = sum g^2      fp32, in a fixed order that depends on the model's size alone (no atomics: the same inputs give the same bits)
 *   norm = sqrtf(s)
 *   c    = (max_norm > 0 && norm > max_norm) ? max_norm / norm : 1.0f          one fp32 division; a select, not a min
 *   Adam consumes g * c (one fp32 multiplication per element; g * 1.0f == g), its arithmetic unchanged.
 *  - max_norm = +inf is "monitor only": the norm is computed and recorded, c = 1, and every step is bit for bit the unclipped one;
 *  - the gradient buffer keeps the RAW gradient: avae_get_grads, avae_grad_buffer and the cost slot are untouched;
 *  - s not finite -- NaN, Inf, or an fp32 overflow of the sum of squares, tested as !(s <= FLT_MAX) -- with skip_nonfinite = 1: the
 *    update is SKIPPED.  theta, m, v and every compute-dtype shadow are not written at all (an early exit, not a multiplication by
 *    0).  A skipped step still consumes its step number: the step counter, lr_t, the eps / corruption keys and the cost history
 *    (which records the step's own, usually NaN, cost) advance exactly as for an applied step; n_skipped counts such steps.  With
 *    skip_nonfinite = 0 the NaN goes through Adam into the parameters, as in TensorFlow;
 *  - the raw norm of every step goes into a device ring of the cost history's depth, indexed like it.
 * max_norm: 0 = no clipping, > 0 (or +inf) = clip by global norm; NaN or negative: an error naming max_norm.  skip_nonfinite: 0 / 1.
 * Both 0 = off (the default): the step is the one it was without this call, no norm is computed, avae_grad_norm_history has nothing.
 * Handle state, set under the handle's mutex; it is not part of avae_save / avae_load.  The call synchronises the device; switching
 * on <-> off captures the step graphs again (on: weight gradients -> sum of squares -> Adam as three launches, never the small nets'
 * fused weight-gradient + Adam launch), changing the values alone does not.  Its device state (the threshold, the per-workgroup
 * partial sums, the norm ring, n_skipped) is allocated by the first call that switches it on and freed by avae_destroy;
 * avae_workspace_bytes is unchanged.  Every training call goes through it -- avae_train_step(s), the masked and _in calls, the
 * library-owned data-parallel pipeline (both buckets' all-reduces then precede the first bucket's Adam) and avae_dp_apply;
 * avae_eval_cost* and every inference call are untouched. */
int avae_set_grad_clip(avae_handle* h, float max_norm, int32_t skip_nonfinite);
/* Raw gradient norms of the most recent n steps (oldest first), the step of the last one and the number of steps skipped since
 * the handle was created.  n may not exceed the history depth (4096) nor the number of steps submitted since clipping was last
 * switched on (error otherwise); n = 0 is fine at any time.  Synchronises the device. */
int avae_grad_norm_history(avae_handle* h, int32_t n, float* host_norms, int64_t* last_step, int64_t* n_skipped);

/* ---- on-device training schedules: KL warm-up (beta annealing, monotone or cyclical), association ramp, learning-rate decay (the
 * reference has none: its coefficients are Python constants, vae_assoc.py:26-31; what a TF-1 caller writes as
 * tf.train.exponential_decay, or a placeholder fed per step).  Every training step has three fp32 multipliers kl_t, a_t, l_t, all 1
 * by default.  With t the step number the update gets (the device step counter + 1 before the step, what avae_get_opt_state
 * reports after it) and u = t - 1:
 *   cost_t   = sum_m w_m [ kl_t * latent_m + recon_m ]  +  lambda_t * sum_pairs assoc
 *   lambda_t = fl32(assoc_lambda * a_t)
 *   lr_eff_t = fl32(learning_rate * l_t)
 *   lr_t     = (float)((double)lr_eff_t * sqrt(1 - beta2^t) / (1 - beta1^t))        Adam's step size, learning_rate replaced
 * and the step's gradient is the gradient of cost_t.  The mean / sum divisors, the presence selects, the denoising inputs and
 * clipping are unchanged.  The KL weight of modality m is (w_m / B_g) * kl_t in this order, so kl_t = 1 gives the unscheduled bits.
 * kl_t is a MULTIPLICATION, not a select: a multiplier of 0 does not hide a non-finite KL term (0 * inf = NaN).  The step's recorded
 * cost (avae_cost_history, the cost returned by the training calls, the data-parallel cost slot) is cost_t.
 * A schedule is a function of the step number alone:
 *   AVAE_SCHED_NONE       1
 *   AVAE_SCHED_PIECEWISE  n_knots in 1..8 knots (knot_step[i], knot_value[i]); knot_step[0] >= 0, strictly increasing; values finite
 *                         and >= 0; period >= 0, and with period > 0: u <- u % period (cyclical annealing), knot_step[last] < period
 *                         required.  Value: knot_value[0] for u <= knot_step[0], knot_value[last] for u >= knot_step[last], else for
 *                         s_i <= u < s_{i+1}
 *                           (float)((double)v_i + ((double)v_{i+1} - (double)v_i) * ((double)(u - s_i) / (double)(s_{i+1} - s_i)))
 *                         without contraction, rounded once: host and device give the same bits
 *   AVAE_SCHED_EXP        (float)pow((double)decay_rate, e),  e = staircase ? (double)(u / decay_steps) : (double)u / (double)decay_steps;
 *                         decay_rate finite and > 0, decay_steps > 0
 * so step t gets the same multipliers alone, inside a 16- or 4-step replay, masked or not, with or without graphs, on every
 * data-parallel rank, and after avae_load / avae_set_opt_state restored the step counter; a step skipped by skip_nonfinite still
 * consumes its number.  The values are evaluated on the device by the staging launch of each submission (no launch is added to
 * the step, the host stays out of the multi-step replays).
 * Evaluation and inference NEVER read a schedule: avae_eval_cost*, avae_score*, avae_loglik*, avae_complete and avae_impute are bit
 * for bit what they are without one (multipliers 1: the configured objective), as for the denoising inputs.
 * avae_set_schedule: NULL or kind AVAE_SCHED_NONE = off for that quantity; all three off is the default.  Errors name the field.
 * Handle state, set under the handle's mutex; not part of avae_save / avae_load.  The call synchronises the device; switching on
 * <-> off (any schedule set <-> none) captures the step graphs again, changing the schedules does not.  Its device state is
 * allocated by the first call that switches it on and freed by avae_destroy; avae_workspace_bytes is unchanged. */
#define AVAE_SCHED_NONE 0
#define AVAE_SCHED_PIECEWISE 1
#define AVAE_SCHED_EXP 2
#define AVAE_SCHED_MAX_KNOTS 8
typedef struct avae_schedule {
    int32_t kind, n_knots;
    int64_t period;
    int64_t knot_step[AVAE_SCHED_MAX_KNOTS];
    float knot_value[AVAE_SCHED_MAX_KNOTS];
    float decay_rate;
    int32_t staircase;
    int64_t decay_steps;
} avae_schedule;
int avae_set_schedule(avae_handle* h, const avae_schedule* kl, const avae_schedule* assoc, const avae_schedule* lr);
/* The multiplier of `schedule` at step number t >= 1 (host only, no GPU; the evaluator the device runs).  NULL schedule: 1.  A
 * failure leaves its message in avae_last_error(NULL). */
int avae_schedule_value(const avae_schedule* schedule, int64_t step, float* out);
/* {kl_t, lambda_t, lr_eff_t} of the most recent n steps (oldest first, host_dst [n][3]) and the step of the last one.  n may not
 * exceed the history depth (4096) nor the number of steps submitted since a schedule was last switched on; n = 0 is fine at any
 * time.  Synchronises the device. */
int avae_hyper_history(avae_handle* h, int32_t n, float* host_dst, int64_t* last_step);

/* ---- parameter averaging: an exponential moving average of the parameters, kept on the device (the reference has none; what a
 * TF-1 caller writes as tf.train.ExponentialMovingAverage(decay[, num_updates]).apply(vars) behind the optimiser, evaluating and
 * serving from the shadow variables).  While it is on, the optimiser launch of every training step, having formed an element's new
 * theta, also moves the element's average e towards it:
 *   e   <- fmaf(theta - e, 1 - d_t, e)                  TF's shadow -= (shadow - var) * (1 - decay): two fp32 roundings, e kept where theta == e
 *   d_t  = warmup ? fminf(decay, (1 + n) / (10 + n)) : decay,   n = (float)t, t the step number the update gets (1 for the first step)
 * d_t depends on the settings and the step number alone: the same bits alone, inside a 16- or 4-step replay, masked or not, with or
 * without graphs, on every data-parallel rank, and after avae_load / avae_set_opt_state restored the step counter.  theta, m, v, the
 * costs and the step counter are bit for bit what they are without averaging.  A step skipped by skip_nonfinite leaves the average
 * alone (and still consumes its number).
 * avae_set_ema: decay in (0, 1) switches averaging on -- the average starts at the current theta -- or, while it is on, changes the
 * settings and keeps the average; decay = 0 switches it off (and switches avae_use_averaged off first).  NaN, decay < 0 or >= 1, and
 * warmup outside {0, 1}: an error naming the argument.  The call synchronises the device; switching on <-> off captures the step
 * graphs again (on: weight gradients -> [sum of squares ->] Adam as separate launches, never the small nets' fused weight-gradient
 * + Adam launch), changing the values alone does not.  The average (one more fp32 array of the parameters' internal size) and its
 * settings are allocated by the first call that switches it on and freed by avae_destroy; avae_workspace_bytes is unchanged.
 * avae_get_ema / avae_set_ema_params: the average in the flat order of avae_get_params, host memory; an error while averaging is off.
 * avae_use_averaged(h, 1): one launch rebuilds every compute-dtype weight shadow from the average; from then on every forward-only
 * entry point (avae_encode ... avae_impute) and avae_eval_cost* run on the averaged parameters, and every call that trains or stages
 * a training step (avae_train_step(s), _masked, _in, avae_stage_batches*, avae_dp_backward, avae_dp_apply) fails with a message naming
 * avae_use_averaged and changes nothing.  avae_use_averaged(h, 0) rebuilds the shadows from theta.  avae_get_params / avae_get_opt_state
 * always return the live state.  avae_set_params and avae_load rebuild the shadows from theta: they leave the handle switched back.
 * Checkpoints: with averaging off avae_save writes the version-2 file; with it on, version 3 = the version-2 body followed by
 * f32 decay | u32 warmup | the average [P] (flat order).  avae_load reads both: a version-3 file switches averaging on with the
 * file's settings and average; a version-2 file loaded while averaging is on restarts the average at the loaded theta. */
int avae_set_ema(avae_handle* h, float decay, int32_t warmup);
int avae_get_ema(avae_handle* h, float* host_dst);
int avae_set_ema_params(avae_handle* h, const float* host_src);
int avae_use_averaged(avae_handle* h, int32_t on);

/* evaluate_cost (vae_assoc.py:388-391): forward + loss, no update. */
int avae_eval_cost(avae_handle* h, const float* const* x_dev, const int32_t* x_ld,
                   const float* eps_dev, float* cost_host, void* stream);
/* transform (vae_assoc.py:393-403): posterior mean (and optionally log-variance) of modality m;
 * any row count. */
int avae_encode(avae_handle* h, int32_t m, const float* x_dev, int32_t x_ld, int32_t rows,
                float* mu_dev, float* logvar_dev, void* stream);
/* generate (vae_assoc.py:405-419): decoder of modality m on fed z [rows, n_z]; any row count. */
int avae_decode(avae_handle* h, int32_t m, const float* z_dev, int32_t rows, float* xhat_dev, void* stream);
/* generate() as the reference's callers use it -- every modality's decoder on the same z (vae_assoc.py:405-419 loops over the
 * modalities; baxter_vae_assoc_writer.py:141-147,259-304 and vae_assoc_model_viewer.py:107-113 call it 10-50 times per search
 * iteration with one live row).  xhat_dev[m] = device [rows, n_input_m] float32, dense.  For 1..64 rows (and for chunks of
 * batch_size rows) the call is one launch that carries the call's pointers by value (it stages z, runs the decoder's first layer of
 * every modality and publishes the pointers to the device) + one replay of a captured graph [remaining decoder launches of all
 * modalities, output launch storing straight into xhat_dev]; conv decoders go through avae_decode's path.  Calls on one handle
 * must be issued on one stream at a time (the published pointers belong to the latest call). */
int avae_generate(avae_handle* h, const float* z_dev, int32_t rows, float* const* xhat_dev, void* stream);
/* reconstruct (vae_assoc.py:421-425): encode -> z = mu + exp(lv/2)*eps -> decode for modality m.
 * eps_dev [rows, n_z] or NULL (internal generator, a fresh draw per call as in the reference). */
int avae_reconstruct(avae_handle* h, int32_t m, const float* x_dev, int32_t x_ld, const float* eps_dev,
                     int32_t rows, float* xhat_dev, void* stream);

/* ---- per-row scoring (the reference has no counterpart: its only figure of merit is the batch cost, vae_assoc.py:388-391).
 * Forward only; M modalities, P = M(M-1)/2 pairs (i<j) in lexicographic order, per row n:
 *   recon[n,m]  Bernoulli -sum_d [x log(1e-3+p) + (1-x) log(1e-3+1-p)], Gaussian 0.5 sum_d (x - x_hat)^2; x_hat / p = decoder m on
 *               z_m = mu_m + exp(lv_m/2) eps[n] (ONE eps row for every modality, as in training)
 *   latent[n,m] -0.5 sum (1 + lv - mu^2 - e^lv)
 *   assoc[n,p]  KL(q_i||q_j) + KL(q_j||q_i) summed over n_z
 *   cost[n]     sum_m w_m (recon + latent) + assoc_lambda sum_p assoc
 *   cross[n,s,d] (AVAE_SCORE_CROSS) the recon loss of modality d decoded from z = mu_s (no noise): source s predicting target d;
 *               the diagonal is deterministic self-reconstruction
 * For rows = batch_size and the same eps the columns give back avae_eval_cost (single replica):
 *   eval_cost == sum_m w_m [mean_n latent + (binary_m ? mean_n recon : sum_n recon)] + assoc_lambda sum_p sum_n assoc */
#define AVAE_SCORE_CROSS 1
/* Host-only (no GPU): columns k of a score row = 1 + 2M + P (+ M*M with AVAE_SCORE_CROSS).  Unknown flags are rejected. */
int avae_score_width(const avae_config* cfg, int32_t flags, int32_t* k);
/* out_dev: device [rows, k] fp32, dense, columns cost | recon[M] | latent[M] | assoc[P] | cross[s*M+d].  Any rows >= 0 (0: no-op),
 * worked in chunks of at most batch_size rows through the inference plans of avae_encode / avae_decode; x_dev[m] as in
 * avae_train_step (x_ld NULL = dense, else x_ld[m] >= n_input).  eps_dev: device [rows, n_z] fp32, or NULL = the internal
 * generator, a fresh draw per call keyed by (seed, draw counter, row of the whole input) as avae_reconstruct's.  As avae_encode,
 * it changes nothing the next training step reads; on a data-parallel replica it scores the local rows, with no collective. */
int avae_score(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, int32_t rows, const float* eps_dev, int32_t flags,
               float* out_dev, void* stream);
/* avae_score for partially paired rows.  present_dev: device uint8 [rows][M], row-major, nonzero = row n has modality m (p below), as
 * in avae_train_steps_masked; NULL is an error (avae_score is the unmasked call).  x_dev[m] == NULL: modality m is absent on every
 * row, whatever its column of present_dev says (never read through).  Everything else -- out_dev, eps_dev, the generator's keys and
 * the per-call draw counter (ONE counter for masked and unmasked calls), rows == 0, chunking, the stream -- is avae_score's.
 *   recon[n,m], latent[n,m]  the unmasked value where p[n,m], else +0.0
 *   assoc[n,(i,j)]           the unmasked value where p[n,i] and p[n,j], else +0.0
 *   cost[n]                  sum_m w_m (recon + latent) + assoc_lambda sum_p assoc over the stored columns (absent addends: +0.0)
 *   cross[n,s,d]             the unmasked value where p[n,s] and p[n,d], else quiet NaN (a zero would read as a perfect prediction)
 * For rows = batch_size and the same eps the columns give back avae_eval_cost_masked, with no need for p:
 *   eval_cost_masked == sum_m w_m [(1/B) sum_n latent + (binary_m ? 1/B : 1) sum_n recon] + assoc_lambda sum_p sum_n assoc
 * Absent entries are selected away, never multiplied by 0 and never read: staging stores zeros for them, the row kernels do not load
 * them, and NaN / Inf / garbage there changes no bit of any output.  Every present output is a select of the unmasked expression:
 * an all-present mask gives avae_score's output bit for bit, and every present column except cost is bitwise avae_score's value for
 * the same rows and eps.  No atomics.  It changes nothing the next training step reads and works on a data-parallel replica as
 * avae_score does; the presence bytes of a chunk (batch_size * M) are staged into a buffer allocated by the first masked scoring
 * call and freed by avae_destroy; avae_workspace_bytes is unchanged. */
int avae_score_masked(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, const uint8_t* present_dev, int32_t rows,
                      const float* eps_dev, int32_t flags, float* out_dev, void* stream);

/* ---- importance-weighted log-likelihoods (IWAE, K = n_samples).  Per row n, proposal s (the encoder of modality s on x_s, as
 * avae_encode gives it), noise eps_k shared by every proposal: z_{s,k} = mu_s + exp(lv_s/2) eps_k (fp32; the decoders read it in the
 * compute dtype), l_d(z) = -recon_d(x_d, dec_d(z)) with avae_score's recon arithmetic (no weights, no 2 pi constant),
 * r_{s,k} = sum_j (-z_j^2/2 + eps_j^2/2 + lv_{s,j}/2) = log N(z; 0, I) - log q_s(z | x_s), LSE_k = log-sum-exp over k:
 *   marginal[s]       LSE_k(l_s(z_{s,k}) + r_{s,k}) - log K                 ~ log p(x_s)
 *   joint[s]          LSE_k(sum_d l_d(z_{s,k}) + r_{s,k}) - log K           ~ log p(x_1..x_M), proposal q_s
 *   conditional[s][d] LSE_k l_d(z_{s,k}) - log K                           ~ log p(x_d | x_s) (diagonal included)
 * out_dev: [rows][2*M + M*M] fp32, row-major: marginal[M] | joint[M] | conditional[M][M] (s-major).
 * eps_dev: [rows][n_samples][n_z] fp32, or NULL for a fresh Philox draw (keyed like avae_score: per-call draw counter, row of the
 * whole input, sample index).  n_samples >= 1; rows == 0 is a no-op.  x_dev / x_ld as avae_score.  Worked in passes of at most
 * batch_size decoded rows (n rows x kb samples); the result depends on batch_size only through the order of the fp32 sums.  As
 * avae_score, it changes nothing the next training step reads; on a data-parallel replica it covers the local rows, with no
 * collective. */
int avae_loglik(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, int32_t rows, int32_t n_samples,
                const float* eps_dev, float* out_dev, void* stream);
/* avae_loglik for partially paired rows; present_dev and x_dev[m] == NULL as in avae_score_masked, the rest as avae_loglik:
 *   marginal[n,s]       the unmasked value where p[n,s], else NaN
 *   conditional[n,s,d]  the unmasked value where p[n,s] and p[n,d], else NaN
 *   joint[n,s]          LSE_k(sum_{d: p[n,d]} l_d(z_{s,k}) + r_{s,k}) - log K where p[n,s], else NaN: the log-likelihood of the
 *                       modalities the row has, under proposal q_s.  The sum starts from 0.0f and adds the present l_d in modality
 *                       order, so a row with only modality s has joint[s] bitwise equal to marginal[s]
 * A row with nothing present is all NaN.  The selection rules, the bitwise ties with the unmasked call (every present output except
 * joint) and the side-effect rules are avae_score_masked's. */
int avae_loglik_masked(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, const uint8_t* present_dev, int32_t rows,
                       int32_t n_samples, const float* eps_dev, float* out_dev, void* stream);

/* ---- gradient latent refinement for partially observed rows (the reference searches z around the encoder's guess by calling
 * generate 10-50 times per iteration from the host, baxter_vae_assoc_writer.py:259-304,466-559; this is the deterministic,
 * gradient-based counterpart, the whole loop on the device).  Per row n independently, z of n_z floats:
 *   J_n(z) = sum_m w_m recon_obs_m(x[n,m], dec_m(z), o[n,m]) + prior_weight * 0.5 * |z|^2
 * dec_m = the decoder of modality m as avae_decode runs it (z read in the compute dtype, fp32 output); o[n,m] an element mask
 * [n_input_m], nonzero = observed; recon_obs_m = avae_score's per-row reconstruction arithmetic summed over the observed elements
 * only (Bernoulli -sum o [x log(1e-3+p) + (1-x) log(1e-3+1-p)], Gaussian 0.5 sum o (x - x_hat)^2); w_m the modality weights.
 * Unobserved elements are selected away, not multiplied by 0: they are never read, NaN / Inf there changes nothing.
 * n_iters updates of per-row, per-element Adam on z in fp32, zero moments at the start, g = dJ_n/dz, t = 1..n_iters:
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  z -= lr (m / (1-b1^t)) / (sqrt(v / (1-b2^t)) + adam_eps)
 * (textbook Adam with bias correction; b1, b2, adam_eps = the config's beta1, beta2, adam_eps).  n_iters = 0 evaluates only.
 *   x_dev[m], x_ld[m]  as avae_score; x_dev[m] == NULL: modality m is unobserved on every row (never read through)
 *   obs_dev            NULL, or obs_dev[m] = device uint8 [rows][n_input_m], dense; NULL: every element of x_dev[m] is observed
 *   z0_dev             device [rows][n_z] fp32, dense: the start
 *   z_dev              device [rows][n_z]: the final z
 *   obj_dev            optional [n_iters+1][rows]: J at z0 and after every update
 *   grad_dev           optional [rows][n_z]: dJ/dz at z0
 *   xhat_dev           optional; xhat_dev[m] optional [rows][n_input_m]: decoder m at the final z (NULL modalities included)
 * rows == 0 is a no-op.  Any row count, worked in chunks of at most batch_size rows on the step's decoder buffers; per chunk one
 * staging launch, then n_iters + 1 passes [decoders forward, masked output gradient + recon_obs, decoder input gradients from the
 * W shadows, update] replayed from captured graphs with no host synchronise in between; the scratch (z, moments, dJ_m/dz) is
 * allocated by the first call and freed by avae_destroy, avae_workspace_bytes is unchanged.  No atomics: the same inputs give
 * bitwise the same outputs.  As avae_score, the call changes nothing the next training step reads (no weight gradient is formed,
 * the gradient buffer is not written); on a data-parallel replica it covers the local rows, with no collective.  MLP decoders
 * only: a model with a conv modality is refused; so are n_iters < 0 and a call whose x_dev[m] are all NULL. */
int avae_complete(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, const uint8_t* const* obs_dev,
                  const float* z0_dev, int32_t rows, int32_t n_iters, float lr, float prior_weight,
                  float* z_dev, float* obj_dev, float* grad_dev, float* const* xhat_dev, void* stream);

/* ---- fused-posterior prediction of missing modalities (the reference's deployed use, image -> joint trajectory,
 * baxter_vae_assoc_writer.py:407-432, is transform on one modality followed by generate; this call uses every modality a row has
 * and also gives the spread of the prediction).  Per row n: S = {m : present[n,m] != 0 and x_dev[m] != NULL}, (mu_m, lv_m) exactly
 * avae_encode's output for modality m.  Fused posterior per latent dimension, fp32, modalities added in index order:
 *   a_m = -lv_m;  A = max_{m in S} a_m;  w_m = exp(a_m - A)
 *   mu_f = (sum_{m in S} w_m mu_m) / (sum_{m in S} w_m);   lv_f = -(A + log((sum_{m in S} w_m) / |S|))
 * -- the precision is the mean of the precisions and the mean is precision-weighted: the minimiser over Gaussians q of
 * sum_{m in S} KL(q || q_m), the divergence training drives to zero.  |S| = 1 is a select: (mu_f, lv_f) are bitwise that modality's
 * avae_encode output.  |S| = 0 is the prior, mu_f = lv_f = +0.0 (the row gets the prior predictive, not NaN).
 * Prediction, for EVERY modality d (for a present one it is a reconstruction):
 *   n_samples = 0       mean_d = dec_d(mu_f), z read in the compute dtype as avae_generate reads it; var_dev is ignored
 *   n_samples = K >= 1  z_k = mu_f + exp(lv_f/2) eps_k (formed as avae_loglik forms it), x_k = dec_d(z_k); mean and population
 *                       variance over k per output element, fp32, sequentially in sample order k = 0..K-1 with Welford's update
 *                         delta = x_k - mean;  mean += delta / (k+1);  M2 += delta * (x_k - mean);  var = M2 / K
 *                       (K = 1: var = +0.0).  The running (mean, M2) is carried per element, so the result does not depend on how
 *                       K is split into passes.
 *   x_dev, x_ld   as avae_score_masked: x_dev[m] == NULL = modality m absent on every row (never offset, no encoder runs)
 *   present_dev   device uint8 [rows][M] as in avae_score_masked, or NULL: every modality with a non-NULL x_dev[m] is present on
 *                 every row
 *   eps_dev       [rows][n_samples][n_z] fp32, or NULL: a fresh Philox draw keyed as avae_loglik's (it advances the ONE per-handle
 *                 draw counter the scoring calls share; a call that decodes no sample draws nothing)
 *   mu_dev, logvar_dev   optional [rows][n_z]: the fused posterior
 *   mean_dev, var_dev    optional; mean_dev[d] / var_dev[d] optional [rows][n_input_d], dense.  A NULL output is skipped.
 * rows == 0 is a no-op; n_samples < 0 is an error.  Any row count: the encoders run on chunks of at most batch_size rows, the
 * decoders in passes of at most batch_size decoded rows laid out as avae_loglik's (input rows x samples, decoded row j*kc + k; a row
 * with more samples than fit spans several passes; K = 0: chunks of batch_size rows).  Through the serve plans up to 16 passes
 * (at most 16 MiB of decoder outputs, held in the call's scratch) share one sampling and one accumulate launch.
 * Absent entries are selected away, never multiplied by 0 and never read: staging stores zeros for them, and NaN / Inf / garbage
 * there changes no bit of any output.  No atomics: the same inputs give bitwise the same outputs.  Conv decoders go modality by
 * modality, as in avae_loglik.  As avae_score, the call changes nothing the next training step reads; on a data-parallel replica
 * it covers the local rows, with no collective.  Its scratch (fused rows, z rows and decoder outputs of one group of passes, the
 * running (mean, M2) of one input row) is allocated by the first call and freed by avae_destroy; avae_workspace_bytes is unchanged. */
int avae_impute(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, const uint8_t* present_dev,
                int32_t rows, int32_t n_samples, const float* eps_dev,
                float* mu_dev, float* logvar_dev, float* const* mean_dev, float* const* var_dev, void* stream);

/* ---- cross-modal retrieval: fused latent distance + top-k (the reference's search cost is a distance of two latent codes evaluated
 * one row at a time on the host, baxter_vae_assoc_writer.py:164-166; this is recall from a memory of encoded examples with no
 * decoder in the loop, and what cross-modal recall@k is computed from).  Queries and gallery are posteriors as avae_encode writes
 * them: device fp32 [rows, n_z] / [gallery_rows, n_z], dense.  Distance of query n and gallery row g, in fp32, the dimensions
 * added in index order j = 0 .. n_z-1 to a sum that starts at +0.0f, with v = expf(lv), iv = expf(-lv) (the precise expf, formed once
 * per row and tile), d = mu_q - mu_g, t = v_q - v_g:
 *   AVAE_METRIC_L2     sum_j d*d                                               sum = fmaf(d, d, sum)
 *   AVAE_METRIC_SYMKL  0.5 * sum_j [ (t*iv_q)*(t*iv_g) + (d*d)*(iv_q + iv_g) ]    sum = fmaf(t*iv_q, t*iv_g, sum); sum = fmaf(d*d, iv_q + iv_g, sum)
 * SYMKL is KL(q_n||q_g) + KL(q_g||q_n), the assoc column of avae_score, rewritten through 0.5 (r + 1/r) - 1 = (v_q - v_g)^2 / (2 v_q v_g)
 * so that every addend is non-negative (no "- n_z" to cancel against), two identical rows give exactly +0.0 and the sum overflows
 * only where the true value does.  The value of a pair is a pure function of the two rows' bits, n_z and the metric: the same
 * bits whichever tile, split or lane formed it, whatever rows, gallery_rows and k are.
 * Result for query n: the first k gallery rows under the total order (isnan(dist), dist, index) ascending -- NaN distances rank
 * behind +Inf, equal floats tie to the lower index.  index_dev [rows, k] int32 and dist_dev [rows, k] fp32, dense; either may be
 * NULL.  A NaN distance is returned as the canonical quiet NaN.  k > gallery_rows fills the tail with index -1, dist +Inf (so
 * gallery_rows == 0 gives nothing else); rows == 0 is a no-op.  With AVAE_METRIC_L2 both log-variance pointers may be NULL and are
 * never read.  Errors (with a message): k < 1, k > AVAE_TOPK_MAX, an unknown metric, rows or gallery_rows < 0, a NULL mu (with rows
 * / gallery_rows > 0), a NULL logvar under SYMKL.
 * No atomics: the result does not depend on rows, on the split count or on the stream.  Two launches per chunk of queries, shaped
 * by avae_latent_topk_plan: k_latent_topk on a grid of query tiles x gallery splits (each workgroup keeps the k best of its slice
 * per query; the rows x gallery_rows matrix never exists in memory) and k_latent_topk_merge over the splits' lists.  The lists
 * live in a scratch allocated by the first call (one allocation of the plan's upper bound, 40 MiB) and freed by avae_destroy;
 * avae_workspace_bytes is unchanged.  As avae_score, the call changes nothing a training step reads, works on any replica with no
 * collective, and inside avae_use_averaged (it only sees latents). */
#define AVAE_METRIC_SYMKL 0
#define AVAE_METRIC_L2    1
#define AVAE_TOPK_MAX     64
int avae_latent_topk(avae_handle* h,
                     const float* q_mu_dev, const float* q_logvar_dev, int32_t rows,
                     const float* g_mu_dev, const float* g_logvar_dev, int32_t gallery_rows,
                     int32_t metric, int32_t k,
                     int32_t* index_dev, float* dist_dev, void* stream);
/* Host-only (no GPU): the launch shapes avae_latent_topk uses.  Queries go in chunks of chunk = min(rows, 16384) rows; per chunk
 * k_latent_topk runs ceil(chunk / query_tile) x n_splits workgroups, split s covering the gallery tiles [s*T, min(tiles, (s+1)*T))
 * of gallery_tile rows each, tiles = ceil(gallery_rows / gallery_tile), T = ceil(tiles / n_splits) -- no split is empty; few
 * queries mean many splits, so that one query against a large gallery still occupies the device.  scratch_bytes = chunk *
 * n_splits * k * 8, at most 40 MiB however many rows.  gallery_rows == 0: n_splits = 0.  Any output pointer may be NULL; k outside
 * [1, AVAE_TOPK_MAX] and negative row counts are errors, the message in avae_last_error(NULL). */
int avae_latent_topk_plan(const avae_config* cfg, int32_t rows, int32_t gallery_rows, int32_t k,
                          int32_t* query_tile, int32_t* gallery_tile, int32_t* n_splits,
                          size_t* scratch_bytes);

/* ---- per-dimension posterior diagnostics: which latent dimensions are alive, where the encoders agree, how far the aggregate
 * posterior is from the prior generate() samples from -- one fused pass over the posteriors of a data set.
 * Inputs: the posteriors of n_mod modalities, 1 <= n_mod <= AVAE_MAX_MODALITIES (n_mod need not be the handle's modality count;
 * n_z is the handle's):
 *   mu_dev[m], logvar_dev[m]   device fp32 [rows, n_z], dense, as avae_encode writes them.  mu_dev[m] == NULL: modality m is
 *                              absent from every row (logvar_dev[m] is then ignored)
 *   present_dev                device uint8 [rows][n_mod], nonzero = row n has modality m, or NULL: every given modality on every row
 * R_sd = the rows that have both s and d, R_mm the rows that have m.  Outputs (device, dense, any may be NULL and is then
 * skipped; a NULL cov also skips the Gram, most of the arithmetic), fp64 except the count, defined in float64 arithmetic on the
 * float32 inputs, means and (co)variances in the population form (divided by the count):
 *   count    [n_mod][n_mod] int64   |R_sd|
 *   mean     [n_mod][n_mod][n_z]    mean of mu_s[:, j] over R_sd
 *   var      [n_mod][n_mod][n_z]    variance of mu_s[:, j] over R_sd; the diagonal [m][m] is the active-units statistic
 *   xcov     [n_mod][n_mod][n_z]    covariance of mu_s[:, j] and mu_d[:, j] over R_sd; the diagonal equals var, bit for bit
 *   assoc    [n_mod][n_mod][n_z]    mean over R_sd of 0.5 * [ (t*iv_s)*(t*iv_d) + (d*d)*(iv_s + iv_d) ], v = expf(lv), iv = expf(-lv),
 *                                   t = v_s - v_d, d = mu_s - mu_d: the per-dimension addend of AVAE_METRIC_SYMKL; diagonal exactly 0
 *   post_var [n_mod][n_z]           mean of expf(lv_m[:, j]) over R_mm
 *   kl       [n_mod][n_z]           mean of 0.5 * (mu^2 + expf(lv) - lv - 1) over R_mm: the per-dimension KL to the prior
 *   cov      [n_mod][n_z][n_z]      covariance matrix of mu_m over R_mm (aggregate posterior covariance = cov + diag(post_var))
 * An empty set has count 0 and NaN everywhere else; rows == 0 is valid and writes exactly that.  A set of one row has var, xcov
 * and cov exactly +0.0 and the row itself as mean.  Absent entries are selected away, never multiplied by 0 and never read: NaN /
 * Inf / garbage there changes no bit of any output.  A non-finite value in a present entry (m, column j) changes only what column
 * j of modality m enters by the definitions: [m][.][j] and [.][m][j] of the tables, post_var[m][j], kl[m][j], row j and column j
 * of cov[m]; every other output keeps the bits it has with that value replaced by 0.
 * Arithmetic: expf in fp32 (the precise one, once per element), everything else in fp64 on values shifted by the column's value in
 * the first row of the set inside the slice, the slices' (count, mean, M2, co-moment) combined in slice order by Chan's formula: the
 * accuracy does not depend on |mean| / std.  The Gram behind cov takes the shifted values rounded to fp32 as factors (products
 * and sums in fp64).  No atomics, one fixed order of every sum: the result is a pure function of the input bits, rows, n_z and the
 * flags -- the same on any stream and on repetition, all-ones flags give the bits of present_dev == NULL -- and the entries [s][d],
 * [m] depend on modalities s, d (m) and their flag columns alone: a call on a subset of the modalities gives the same bits for
 * the entries it shares with the full call (the row partition is a function of rows alone).
 * Errors (with a message naming the argument, outputs untouched): n_mod outside [1, AVAE_MAX_MODALITIES], rows < 0, a NULL out, a
 * NULL mu_dev array, a non-NULL mu_dev[m] with a NULL logvar_dev[m].  Asynchronous on `stream`.  Two launches, shaped by
 * avae_latent_stats_plan: k_latent_stats on a grid of row slices x work items (one item per modality, one per pair s < d), one
 * partial per (slice, item) to a scratch, and k_latent_stats_merge.  The scratch is allocated by the first call (one allocation
 * of the plan's upper bound: 256 slices, 4 modalities, n_z = 64 -- 42,487,808 bytes) and freed by avae_destroy;
 * avae_workspace_bytes is unchanged.  As avae_latent_topk, the call changes nothing a training step reads, works on any replica
 * with no collective, and inside avae_use_averaged (it only sees latents). */
typedef struct avae_latent_stats_out {      /* device pointers, dense, any may be NULL */
    int64_t* count;
    double *mean, *var, *xcov, *assoc, *post_var, *kl, *cov;
} avae_latent_stats_out;
int avae_latent_stats(avae_handle* h, int32_t n_mod,
                      const float* const* mu_dev, const float* const* logvar_dev,
                      const uint8_t* present_dev, int32_t rows,
                      const avae_latent_stats_out* out, void* stream);
/* Host-only (no GPU): the row partition avae_latent_stats uses, a function of rows alone.  Slice i covers the rows
 * [i * row_tile, min(rows, (i + 1) * row_tile)); row_tile = max(256, ceil(rows / 256) rounded up to a multiple of 64), so there are
 * at most 256 slices, none empty, and n_slices == 0 only for rows == 0.  scratch_bytes = n_slices * (M * (1 + 5 n_z + n_z^2) +
 * M (M - 1) / 2 * (1 + 8 n_z)) * 8 for the configuration's M = n_modalities and n_z: at most 42,487,808.  Any output pointer may be
 * NULL; rows < 0 is an error, the message in avae_last_error(NULL). */
int avae_latent_stats_plan(const avae_config* cfg, int32_t rows, int32_t* row_tile, int32_t* n_slices,
                           size_t* scratch_bytes);

/* ---- aggregate-posterior log-density: log q_agg(z), q_agg(z) = 1/G' sum_g q(z | x_g), the mixture of a gallery's posteriors, and
 * its per-dimension marginals, as one streamed log-sum-exp.  It is what the ELBO decomposition KL = index-code
 * MI + total correlation + dimension-wise KL (Hoffman & Johnson 2016, Chen et al. 2018), the divergence of two encoders' aggregate
 * posteriors and a leave-one-out novelty score are computed from.
 *   z_dev                    query points, device fp32 [rows, n_z], dense
 *   g_mu_dev, g_logvar_dev   the gallery's posteriors as avae_encode writes them, device fp32 [gallery_rows, n_z], dense
 *   exclude_dev              device int32 [rows] or NULL.  E_n = the gallery rows counted for query n: every row, minus row
 *                            exclude[n] when 0 <= exclude[n] < gallery_rows (any other value excludes nothing); G' = |E_n|
 *   joint_dev                device fp32 [rows] or NULL;  marginal_dev  device fp32 [rows, n_z] or NULL
 * With c = 0.5 log(2 pi):
 *   l(n,g,j)      = -0.5 (lv_gj + (z_nj - mu_gj)^2 exp(-lv_gj))
 *   marginal[n,j] = log sum_{g in E_n} exp(l(n,g,j))        - log G' - c
 *   joint[n]      = log sum_{g in E_n} exp(sum_j l(n,g,j))  - log G' - n_z c
 * Arithmetic: iv = expf(-lv) (the precise expf, formed once per gallery element while staging), d = z - mu,
 * l = -0.5f * fmaf(d*d, iv, lv) (evaluated as fmaf(d*d, -0.5f*iv, -0.5f*lv): the same bits, a scaling by a power of two); the joint
 * exponent is the sum of l over j = 0 .. n_z-1 in index order, added to +0.0f.  The log-sum-exp is a running (max, sum scaled by it)
 * in fp32 per query and per column: gallery rows join in blocks of 8 -- rows [8b, 8b+8) of the gallery -- the block's max against
 * the running max, one rescale, the 8 exponentials exp(l - max) added in row order; the exponential inside the sums is the hardware
 * exp2 on the argument times log2(e).  Marginals take the blocks of a slice in order; the joint keeps one running pair per block
 * position b mod 8 and combines the 8 in position order when the slice is done.  The merge launch combines the slices' pairs in
 * slice order in fp64, subtracts log G' and the constant in fp64 and rounds once to fp32.
 * Edges, by the definition: a query whose every term is -Inf gives -Inf, not NaN; a gallery row with lv = +Inf contributes 0;
 * G' = 0 (gallery_rows == 0, or gallery_rows == 1 with that row excluded) gives NaN, "no estimate"; rows == 0 is a no-op.  A NaN at
 * gallery (g, j) makes marginal[n, j] and joint[n] NaN for every query that counts row g and changes no other output bit; a NaN at
 * z[n, j] changes marginal[n, j] and joint[n] only.  An excluded row is selected away, never multiplied by 0: NaN / Inf / garbage in
 * it changes no bit of that query's outputs.  A NULL marginal_dev skips the per-dimension sums (n_z of the n_z + 1 exponentials per
 * pair), a NULL joint_dev the joint sum; both NULL is an error.
 * Errors (with a message naming the argument, outputs untouched): rows or gallery_rows < 0, a NULL z_dev with rows > 0, a NULL
 * g_mu_dev or g_logvar_dev with gallery_rows > 0, joint_dev and marginal_dev both NULL.
 * No atomics; the gallery partition is a function of gallery_rows alone: the result for a query does not depend on rows, on the
 * query's position in the call, on the stream or on repetition, and joint is the same bits with or without marginal_dev (and the
 * other way round).  Two launches per chunk of queries, shaped by avae_agg_logpdf_plan: k_agg_logpdf on a grid of query tiles x
 * gallery slices and k_agg_logpdf_merge.  The slices' pairs live in a scratch allocated by the first call (one allocation of the
 * plan's upper bound, 68,157,440 bytes) and freed by avae_destroy; avae_workspace_bytes is unchanged.  As avae_latent_topk, the call
 * changes nothing a training step reads, works on any replica with no collective, and inside avae_use_averaged (it only sees
 * latents). */
int avae_agg_logpdf(avae_handle* h,
                    const float* z_dev, int32_t rows,
                    const float* g_mu_dev, const float* g_logvar_dev, int32_t gallery_rows,
                    const int32_t* exclude_dev,
                    float* joint_dev, float* marginal_dev, void* stream);
/* Host-only (no GPU): the launch shapes avae_agg_logpdf uses.  slice_rows = max(1024, ceil(gallery_rows / 64) rounded up to a
 * multiple of 64) and n_slices = ceil(gallery_rows / slice_rows) -- at most 64 slices, none empty, a function of gallery_rows alone;
 * gallery_rows == 0: n_slices = 0.  Queries go in chunks of chunk_rows = min(rows, 2048); per chunk k_agg_logpdf runs
 * ceil(chunk / query_tile) x n_slices workgroups.  scratch_bytes = chunk_rows * n_slices * (1 + n_z) * 8 for the configuration's
 * n_z: at most 68,157,440.  Any output pointer may be NULL; negative row counts are errors, the message in avae_last_error(NULL). */
int avae_agg_logpdf_plan(const avae_config* cfg, int32_t rows, int32_t gallery_rows,
                         int32_t* query_tile, int32_t* chunk_rows, int32_t* slice_rows, int32_t* n_slices,
                         size_t* scratch_bytes);

/* ---- mixture prior fitted to the posteriors: p(z) = sum_k pi_k N(z; m_k, diag exp(s_k)), 1 <= K <= 64, fitted after training to
 * the encoders' posteriors q_n = N(mu_n, diag v_n), v_n = exp(logvar_n), by EM on the Jensen lower bound of
 * 1/N sum_n E_{q_n}[log p(z)] (ex-post density estimation, Ghosh et al. 2020).  It is what replaces the
 * N(0, I) draw of avae_generate's caller when the aggregate posterior is a handful of clusters, and it is an unsupervised
 * clustering of the codes.
 *   mu_dev, logvar_dev   the posteriors as avae_encode writes them, device fp32 [rows, n_z], dense; logvar_dev NULL: points, v = 0
 *   weights_dev [K], means_dev [K, n_z], logvars_dev [K, n_z]   device fp32, dense; avae_gmm_fit: in the initial, out the fitted
 *   bound_dev            device fp64 [n_iters + 1]: bound[t] is the bound of the parameters ENTERING iteration t, bound[n_iters] that
 *                        of the returned ones (a last pass that only scores)
 *   n_used_dev           device int32 [1]: the rows counted
 * One iteration, over the used rows (a row with any non-finite mu or logvar entry is skipped, never added to a sum):
 *   E_nk  = log pi_k - 1/2 sum_j [log 2pi + s_kj + ((mu_nj - m_kj)^2 + v_nj) exp(-s_kj)]
 *   ll_n  = logsumexp_k E_nk,  r_nk = exp(E_nk - ll_n),  bound = mean ll_n
 *   R_k = sum r_nk,  S1_kj = sum r_nk (mu_nj - m_kj),  S2_kj = sum r_nk ((mu_nj - m_kj)^2 + v_nj)
 *   pi_k = R_k / sum_k R_k,  m'_kj = m_kj + S1_kj / R_k,  s'_kj = log max(S2_kj / R_k - (S1_kj / R_k)^2, var_floor)
 * The sums are shifted by the CURRENT mean, so the variance never comes from a difference of large numbers.  A component with
 * R_k < 1e-8 keeps its mean and log-variance and gets the weight R_k / sum R (no re-seeding).  With no used row the parameters stay
 * as given and the bound is NaN; rows == 0 is that case, not an error.  n_iters == 0 scores the initial parameters and leaves them
 * untouched.  There is no early stop: the caller reads bound.
 * Arithmetic: the exponent is c_k = logf(pi_k) - 0.5f * sum_j (s_kj + log 2pi) followed by the chain
 * E = fmaf(fmaf(d, d, v), -0.5f * expf(-s_kj), E), d = mu_nj - m_kj, over j = 0 .. n_z-1 in index order; v = expf(logvar) formed
 * once per element; p_k = expf(E_k - max_k E_k), ll = max + logf(sum), r_k = p_k / sum -- all fp32 but sum, the p_k added in k
 * order in fp64 and rounded to fp32 once, so that a row of r sums to 1 within 2^-23 for every K.  The
 * sums of r d, r (d^2 + v) and r run in fp64 over a slice's rows in row order (d = mu_nj - m_kj formed in fp64 here, fused
 * multiply-adds: the products are exact, so S2 / R - (S1 / R)^2 loses nothing to the rounding of d^2), ll is added
 * in fp64 (per row position of the tiles, the 64 positions in order at the end of a slice); a skipped row is selected away, it
 * enters every sum as +-0; the slices' partials are combined in slice order and the update is evaluated in fp64, then rounded to fp32:
 * the parameters are fp32 between iterations, so a fit of a iterations continued for b more from its own output gives the bits
 * of a fit of a + b.  No atomics, one fixed order of every sum; the row partition is a function of rows alone (avae_gmm_plan):
 * the result is a pure function of the input bits -- the same on any stream and on repetition.
 * The whole loop is enqueued on `stream` with no host synchronisation inside: two launches per iteration (k_gmm_estep on a grid
 * of row slices, one partial per slice to a scratch; k_gmm_mstep, one thread per (k, j)) and two for the last scoring pass.  The scratch
 * is allocated by the first call (one allocation of the plan's upper bound, 16,978,432 bytes) and freed by avae_destroy;
 * avae_workspace_bytes is unchanged.
 * Errors (with a message naming the argument, outputs untouched): rows < 0, n_components outside [1, 64], n_iters < 0, var_floor
 * <= 0 or not finite, a NULL mu_dev with rows > 0, a NULL weights_dev / means_dev / logvars_dev / bound_dev / n_used_dev.
 * As avae_latent_topk, the calls change nothing a training step reads, work on any replica with no collective, and inside
 * avae_use_averaged (they only see latents). */
int avae_gmm_fit(avae_handle* h,
                 const float* mu_dev, const float* logvar_dev, int32_t rows,
                 int32_t n_components, int32_t n_iters, float var_floor,
                 float* weights_dev, float* means_dev, float* logvars_dev,
                 double* bound_dev, int32_t* n_used_dev, void* stream);
/* The E-step alone, with per-row outputs: ll_dev fp32 [rows] = ll_n (for points exactly log p(z)), component_dev int32 [rows] = the
 * argmax of r_n. (ties to the lower index), resp_dev fp32 [rows, K] = r_nk.  Any output may be NULL, not all of them.  A skipped
 * (non-finite) row gives ll = NaN, component = -1, resp = NaN.  A row's outputs are a pure function of its own bits and the
 * parameters: they do not depend on the other rows, on which outputs are asked for, on the stream or on repetition, and ll is
 * the number avae_gmm_fit averages into bound.  rows == 0 is a no-op.  Errors: rows < 0, n_components outside [1, 64], a NULL
 * mu_dev with rows > 0, a NULL weights_dev / means_dev / logvars_dev, all three outputs NULL.  One launch of k_gmm_estep. */
int avae_gmm_score(avae_handle* h,
                   const float* mu_dev, const float* logvar_dev, int32_t rows, int32_t n_components,
                   const float* weights_dev, const float* means_dev, const float* logvars_dev,
                   float* ll_dev, int32_t* component_dev, float* resp_dev, void* stream);
/* Host-only (no GPU): the row partition both calls use, a function of rows alone.  Slice i covers the rows
 * [i * slice_rows, min(rows, (i + 1) * slice_rows)); slice_rows = max(64, ceil(rows / 256) rounded up to a multiple of 64), so
 * there are at most 256 slices, each a whole number of 64-row tiles (the last one apart), none empty, and n_slices == 0 only for
 * rows == 0.  scratch_bytes = n_slices * (2 + K + 2 K n_z) * 8 + 2 * (K + 2 K n_z) * 4 for the configuration's n_z: at most
 * 16,978,432.  Any output pointer may be NULL; rows < 0 or n_components outside [1, 64] is an error, the message in
 * avae_last_error(NULL). */
int avae_gmm_plan(const avae_config* cfg, int32_t rows, int32_t n_components,
                  int32_t* slice_rows, int32_t* n_slices, size_t* scratch_bytes);

/* ---- 2-D t-SNE map of the posteriors (van der Maaten & Hinton 2008): where the codes of every modality lie,
 * as a picture.  The affinities are built from avae_latent_topk's metric -- under AVAE_METRIC_SYMKL from the divergence the
 * association term is trained on, variances included -- and the N x N matrix never exists: p_ij is recomputed in every iteration
 * from the pair's distance and three numbers per row.
 *   mu_dev, logvar_dev   the posteriors as avae_encode writes them, device fp32 [rows, n_z], dense.  AVAE_METRIC_L2 never reads
 *                        logvar_dev (it may be NULL: points)
 * D_ij is the distance of rows i and j exactly as avae_latent_topk states it (the same chain of fused multiply-adds over
 * j = 0 .. n_z-1 from +0.0f, v = expf(lv), iv = expf(-lv) formed once per row and tile): one device function serves the
 * calibration and the force pass, so D_ij has the same bits in both, D_ij == D_ji, and D_ij - min_j D_ij >= 0.
 * A row with a non-finite mu (or, under SYMKL, logvar) entry is skipped: it is selected away, never multiplied by 0, it enters
 * every sum as +-0, its outputs are NaN and no bit of another row's output depends on what it held.  F = the used rows.
 *
 * avae_embed_calibrate: per used row i the search for beta_i with entropy log(perplexity).
 *   m_i = min_{j != i} D_ij,  e_ij = expf(-(beta_i * (D_ij - m_i))),  S0_i = sum_{j != i} e_ij,  S1_i = sum (D_ij - m_i) e_ij,
 *   H_i = log S0_i + beta_i S1_i / S0_i
 * beta starts at 1; while |H - log(perplexity)| > tol and fewer than max_tries values were tried: H too large -> the lower bound
 * becomes beta and beta = 2 beta (no upper bound yet) or (beta + upper) / 2; else the upper bound becomes beta and beta = beta / 2
 * (no lower bound yet) or (beta + lower) / 2.  beta stays inside [2^-100, 2^100].  Outputs, device, dense [rows] (NaN / 0 tries on
 * a skipped row, and on every row when F < 2): beta_dev, shift_dev = m_i, norm_dev = S0_i AT the returned beta_i (all fp32),
 * tries_dev int32 = the values tried; n_used_dev int32 [1] = F.  A row's (beta, shift, norm, tries) is a function of its own
 * distances, in row order, alone.  Arithmetic: e and (D - m) e in fp32, added in fp32 over the 4 columns a thread holds of a
 * 64-row tile, in fp64 over the tiles in order and over the 16 threads of a row (a fixed tree); H and the comparison in fp64;
 * beta and its bounds are fp32.  One workgroup owns 64 rows and streams all rows once for the minima and once per try
 * (O(rows^2 x tries): rows <= 65,536); finished rows freeze.
 *
 * avae_embed_iterate: n_iters iterations of gradient descent on KL(P || Q) from the state (y, vel, gain), device fp32 [rows, 2]
 * each, updated in place.  With c_i = 1 / (2 F norm_i):
 *   p_ij = e_ij c_i + e_ji c_j  (i != j; two fp32 products and their sum: p_ij == p_ji bit for bit),  p_ii = 0
 *   w_ij = 1 / (1 + |y_i - y_j|^2),  w_ii = 0,  Z = sum_{i != j} w_ij
 *   A_i = sum_j p_ij w_ij (y_i - y_j),  R_i = sum_j w_ij^2 (y_i - y_j),  grad_i = 4 (alpha A_i - R_i / Z)
 *   KL = sum_{p_ij > 0} p_ij (log p_ij - log w_ij) + log Z      (always with the unexaggerated p)
 * Iteration t = it0 + s (s = 0 .. n_iters-1): alpha = early_exaggeration and mom = momentum0 while t < exaggeration_iters, then
 * alpha = 1 and mom = momentum1; per element  gain = ((grad > 0) != (vel > 0)) ? gain + 0.2 : gain * 0.8,  gain = max(gain, 0.01),
 * vel = mom vel - lr gain grad,  y += vel  (evaluated in fp64 from the fp32 state and the fp64 gradient; gain, vel and y each rounded
 * to fp32 once).  kl_dev fp64 [n_iters + 1]: kl[s] belongs to the Y ENTERING iteration it0 + s, kl[n_iters] to the returned Y (a last
 * pass that only evaluates); n_iters == 0 evaluates and leaves y, vel and gain untouched.  grad_dev: NULL, or fp32 [rows, 2], the
 * gradient at the entering Y of the call's first pass (no other output bit depends on it being asked for).  The forces are
 * translation invariant and the map is not centred inside the loop; with center != 0 (and n_iters > 0) a last launch subtracts the
 * mean of the used rows of the returned Y (fp64, fixed order).  A skipped row's y, vel, gain and grad come back NaN; with F < 2
 * kl is NaN and the used rows' state stays as given.
 * Arithmetic: everything per pair in fp32 (expf, logf and the division are the precise ones), added in fp32 over the 4 columns a
 * thread holds of a tile, in fp64 over the tiles of a split in order and over the 16 threads of a row (a fixed tree); the splits in
 * split order, Z and the KL (thread t of a block the rows t, t + 256, ..., then the 256 sums in order), the gradient and the
 * update in fp64.  sum p log p does not depend on Y: the first pass of a call forms it and the later ones reuse it.
 * The state is fp32 between iterations, so a iterations followed by b more from the returned (y, vel, gain) with it0 = a give the
 * bits of a + b iterations run with center = 0.  No atomics, one fixed order of every sum; the split plan is a function of rows
 * alone (avae_embed_plan): the outputs are a pure function of the input bits -- the same on any stream and on repetition.
 * The whole loop is enqueued on `stream` with no host synchronisation inside: k_embed_scan once, then two launches per pass
 * (k_embed_forces on a grid of row tiles x splits, one partial per (row, split) to a scratch; k_embed_update).  The scratch is
 * allocated by the first call of either entry (one allocation of the plan's upper bound, 7,406,720 bytes) and freed by
 * avae_destroy; avae_workspace_bytes is unchanged.
 * rows == 0 is a no-op.  Errors (with a message naming the argument, outputs untouched): rows < 0 or > 65,536, an unknown metric,
 * perplexity outside [1, rows - 1], tol <= 0, max_tries < 1, n_iters < 0, it0 < 0, learning_rate <= 0 or not finite, a NULL
 * mu_dev, a NULL logvar_dev under SYMKL, any other NULL pointer but grad_dev.
 * As avae_latent_topk, the calls change nothing a training step reads, work on any replica with no collective, and inside
 * avae_use_averaged (they only see latents). */
int avae_embed_calibrate(avae_handle* h,
                         const float* mu_dev, const float* logvar_dev, int32_t rows, int32_t metric,
                         double perplexity, double tol, int32_t max_tries,
                         float* beta_dev, float* shift_dev, float* norm_dev, int32_t* tries_dev,
                         int32_t* n_used_dev, void* stream);
int avae_embed_iterate(avae_handle* h,
                       const float* mu_dev, const float* logvar_dev, int32_t rows, int32_t metric,
                       const float* beta_dev, const float* shift_dev, const float* norm_dev,
                       float* y_dev, float* vel_dev, float* gain_dev,
                       int32_t it0, int32_t n_iters, float learning_rate,
                       float early_exaggeration, int32_t exaggeration_iters, float momentum0, float momentum1,
                       int32_t center, double* kl_dev, float* grad_dev, void* stream);
/* Host-only (no GPU): the launch shapes of k_embed_forces, a function of rows alone.  tiles = ceil(rows / row_tile) tiles of
 * row_tile = 64 rows; the streamed side is cut into n_splits = ceil(tiles / tiles_per_split) splits of tiles_per_split =
 * ceil(tiles / min(tiles, ceil(1024 / tiles))) tiles -- about 1024 workgroups, so small inputs are split too (32 tiles: 32 splits
 * of one); split s covers the tiles [s * tiles_per_split, min(tiles, (s + 1) * tiles_per_split)), none is empty; rows == 0:
 * n_splits = 0.  scratch_bytes = 66,688 + 7 * rows * n_splits * 8 (rows * n_splits <= 131,072).  Any output pointer may be NULL;
 * rows < 0 or > 65,536 is an error, the message in avae_last_error(NULL). */
int avae_embed_plan(const avae_config* cfg, int32_t rows,
                    int32_t* row_tile, int32_t* n_splits, int32_t* tiles_per_split, size_t* scratch_bytes);

/* ---- motion decoding: the joint modality's rows as joint trajectories.  A row of the joint modality holds
 * P = D * Kb standardised parameters of the reference's function approximator, D joints x (Kb - 1 basis weights + 1 offset), row-major
 * [D][Kb] (baxter_writer.py:53-82, baxter_vae_assoc_writer.py:109-111); after every generate the reference un-normalises them,
 * evaluates the approximators over the phase points and clamps to the joint limits (baxter_vae_assoc_writer.py:145-150, 439-458,
 * pyrbf_funcapprox.py:123-143), and its training data are least-squares fits of the same basis (pyrbf_funcapprox.py:104-121).  The
 * device sees only matrices (vae_assoc_amd/motion.py builds them on the host).  Dense device fp32 everywhere but saturated_dev
 * (int32); trajectories are [rows][T][D].
 *   theta[r][d][k] = params[r][d*Kb + k] * scale[d*Kb + k] + shift[d*Kb + k]        (one fma; NULL scale / shift: 1 / 0)
 *   q[r][t][d]     = sum_k phi[t][k] theta[r][d][k]  (+ sum_c anchor_gain[t][c] anchor_target[r][d][c])
 * every sum an fp32 fma chain in index order from 0, then q is clamped to [limits[d][0], limits[d][1]] for each joint whose upper
 * limit is above its lower one -- by comparison, so a NaN stays NaN.  A linear equality constraint of the reference
 * (pyrbf_funcapprox.py:41-61) is theta -> A theta + B target: the caller passes phi already multiplied by A and anchor_gain =
 * phi_raw B, the kernels know nothing of constraints.
 * avae_motion_eval: traj_dev = q; saturated_dev[r][d] = the number of clamped points; with a reference, rmse_dev[r][d] =
 *   sqrt(mean_t (q - q_ref)^2) and maxabs_dev[r][d] = max_t |q - q_ref| (NaN if any difference is).  The reference is ref_traj_dev as
 *   it is, or ref_params_dev evaluated by the same code with the same scale, shift and limits and no anchor -- the bits eval gives for
 *   those parameters.  Every output may be NULL, but not all; the error outputs need a reference; both references is an error.
 * avae_motion_fit: theta[r][d][:] = pinv [Kb][T] times traj[r][:][d] (t ascending), params_out = (theta - shift) / scale.
 * avae_motion_moments: each of a row's S samples [rows][S][P] is evaluated exactly as by avae_motion_eval, clamp included, and folded
 *   in sample order into a per-element running mean and M2 by the sequential update of avae_impute (delta = x - mean;
 *   mean += delta / (k + 1); M2 += delta * (x - mean), the last an fma); var = M2 / S (population variance); saturated_frac[r][d] =
 *   clamped points over all samples / (S * T).  The [rows][S][T][D] values are never stored.  S = 1: var is 0 and the mean is
 *   avae_motion_eval's trajectory, bit for bit.
 * rows == 0 is a no-op.  Errors (message in avae_last_error, nothing launched): rows < 0, D outside [1, 16], Kb outside [1, 64], T
 * outside [1, 1024], nc outside [0, 4], S < 1, a NULL required pointer (anchor_gain / anchor_target with nc > 0 included).
 * No atomics, one fixed order of every sum, and a workgroup's work is a function of its own rows alone: a row's outputs are a pure
 * function of its bits and the matrices -- the same alone or among other rows, on any stream, on repetition and whichever optional
 * outputs are asked for; a non-finite parameter affects only its own (row, joint).  One launch each, no scratch, nothing of the
 * handle is read or written: the calls change nothing a training step reads, work on any replica with no collective, and inside
 * avae_use_averaged. */
int avae_motion_eval(avae_handle* h, const float* params_dev, int32_t rows, int32_t D, int32_t Kb, int32_t T,
                     const float* phi_dev, const float* scale_dev, const float* shift_dev, const float* limits_dev,
                     const float* anchor_gain_dev, const float* anchor_target_dev, int32_t nc,
                     const float* ref_traj_dev, const float* ref_params_dev,
                     float* traj_dev, int32_t* saturated_dev, float* rmse_dev, float* maxabs_dev, void* stream);
int avae_motion_fit(avae_handle* h, const float* traj_dev, int32_t rows, int32_t D, int32_t Kb, int32_t T,
                    const float* pinv_dev, const float* scale_dev, const float* shift_dev, float* params_dev, void* stream);
int avae_motion_moments(avae_handle* h, const float* samples_dev, int32_t rows, int32_t S, int32_t D, int32_t Kb, int32_t T,
                        const float* phi_dev, const float* scale_dev, const float* shift_dev, const float* limits_dev,
                        const float* anchor_gain_dev, const float* anchor_target_dev, int32_t nc,
                        float* mean_dev, float* var_dev, float* saturated_frac_dev, void* stream);

/* ---- pen-path kinematics and stroke rendering: from a joint trajectory to the picture it writes.  The
 * reference turns every predicted trajectory into a Cartesian pen path, one PyKDL call per time point
 * (baxter_vae_assoc_writer.py:448-449), draws it with matplotlib, crops the drawing to its ink and shrinks it to 28 x 28 with OpenCV
 * (utils.py:240-257), and compares that picture with the one the robot was shown (baxter_vae_assoc_writer.py:344-399).  These two
 * calls are the project's own definition of that picture, not a bit copy of Agg and cv2.INTER_AREA.  Dense device fp32 everywhere.
 * avae_motion_fk: path[r][t] = the tip of a serial chain of D revolute joints at the angles traj[r][t][:],
 *   T(q) = F_0 Rot(axis_0, q_0) F_1 Rot(axis_1, q_1) ... F_{D-1} Rot(axis_{D-1}, q_{D-1}) F_D,  tip = T[:3, 3],
 *   frames_dev [D + 1][3][4] the fixed transforms between the joints (rotation | translation, vae_assoc_amd/kinematics.py packs them
 *   from URDF-style joints), axes_dev [D][3] unit vectors, Rot Rodrigues' formula with the precise sincosf; the operations and their
 *   order are written in csrc/avae_render.h.
 * avae_stroke_render: a row's path p_t, t < T, drawn as a line of half width half_width with round caps and joins:
 *   c_t = (u . (p_t - mean), v . (p_t - mean)) with plane_dev [3][3] = rows u, v, n and mean the mean over t; the ink box lo = min_t
 *   c_t - half_width, hi = max_t c_t + half_width (exact), its centre ctr and longer side L; the window W = (1 + margin) L, sampled
 *   on a grid of pitch delta = W / (H ss): sample (a, b), a, b < H ss, lies at u = ctr_u - W / 2 + (b + 1/2) delta, v = ctr_v + W / 2 -
 *   (a + 1/2) delta (image row 0 is the top); its coverage is clamp(1/2 + (half_width - d) / delta, 0, 1) with d its distance to the
 *   polyline (the minimum over the T - 1 segments, the foot clamped to the segment; a segment shorter than 1e-15 is a point, T = 1 a
 *   dot); image[r][i * H + j] is the mean of the ss x ss coverages of pixel (i, j).  window[r] = (ctr_u, ctr_v, W).  With
 *   target_dev, img_l2[r] = sqrt(sum (image - target)^2); with height_dev, height_l2[r] = sqrt(sum_t (n . p_t - height[r])^2).
 *   Every sum has one fixed order (csrc/avae_render.h writes it down); pixels that cannot hold ink are skipped, which changes no bit.
 *   A row whose path holds a non-finite value gets NaN in every output and touches no other row.
 * rows == 0 is a no-op.  Errors (message in avae_last_error, nothing launched): rows < 0, D outside [1, 16], T outside [1, 1024],
 * H outside [1, 64], ss not 1, 2, 4 or 8, half_width not > 0, margin not >= 0, a NULL required pointer, every output NULL, img_l2_dev
 * without target_dev, height_l2_dev without height_dev.
 * One launch each, no atomics, no scratch, nothing of the handle is read or written: a row's outputs are a pure function of its
 * bits and the constants -- the same alone or among other rows, on any stream, on repetition and whichever optional outputs are
 * asked for -- and the calls work on any replica and inside avae_use_averaged. */
int avae_motion_fk(avae_handle* h, const float* traj_dev, int32_t rows, int32_t T, int32_t D,
                   const float* frames_dev, const float* axes_dev, float* path_dev, void* stream);
int avae_stroke_render(avae_handle* h, const float* path_dev, int32_t rows, int32_t T, const float* plane_dev,
                       float half_width, float margin, int32_t H, int32_t ss,
                       const float* target_dev, const float* height_dev,
                       float* image_dev, float* window_dev, float* img_l2_dev, float* height_l2_dev, void* stream);

/* ---- gradients through the writing chain: the vector-Jacobian products of avae_stroke_render, avae_motion_fk
 * and avae_motion_eval, and a batched Adam step, so that a motion can be moved towards the picture it should write by descent instead
 * of by search.  Dense device fp32 everywhere but t_dev / status_dev (int32).
 * avae_stroke_render_vjp: the inputs of avae_stroke_render and the cotangents g_image_dev [rows][H * H], g_img_l2_dev [rows],
 *   g_height_l2_dev [rows] (each optional) -> grad_path_dev [rows][T][3], the gradient of  sum g_image . image + g_img_l2 img_l2 +
 *   g_height_l2 height_l2  with respect to the path.  In the notation above (alpha_b = (b + 1/2) / (H ss) - 1/2):
 *   a pixel's cotangent is g_image + g_img_l2 (image - target) / img_l2 (the second term 0 where img_l2 == 0), a sample's g_cov that
 *   over ss^2.  A sample counts only in the open linear zone 0 < x < 1 of x = 1/2 + (half_width - d) / delta; there g_d = -g_cov /
 *   delta, and -(half_width - d) / delta^2 g_cov goes to g_delta.  With j the first segment that attains the sample's distance, tau
 *   its clamped foot parameter (0 for a segment that is a point) and n = (sample - foot) / d (0 where d == 0):  g_s = g_d n,
 *   c_j gets -(1 - tau) g_s, c_{j+1} gets -tau g_s, g_ctr = sum g_s, g_W = sum (g_s.u alpha_b - g_s.v alpha_a) + g_delta / (H ss).
 *   g_ctr / 2 goes to the first point with the largest and to the first with the smallest c on each axis, (1 + margin) g_W to the
 *   first argmax of the longer axis and its negative to the first argmin (u on a tie).  grad_path_t = g_c[t] . (u, v) + g_height_l2
 *   (n . p_t - height) / height_l2 n (0 where height_l2 == 0); the mean drops out because sum_t g_c[t] = 0.  T = 1: the image part is
 *   exactly 0.  image_dev, window_dev, img_l2_dev, height_l2_dev (each optional) receive the forward outputs, bitwise
 *   avae_stroke_render's; objective_dev [rows] (optional) g_img_l2 img_l2 + g_height_l2 height_l2.  A row with a non-finite
 *   coordinate is NaN in its own outputs; a non-finite cotangent makes the image part of its own row NaN.  The per-point sums are
 *   64-bit fixed-point integers at a scale taken from the row's own cotangents (csrc/avae_grad.h): a row's grad_path is the same
 *   bits alone or among other rows, on any stream, on repetition and whichever optional outputs are asked for.
 * avae_motion_fk_vjp: grad_traj[r][t][j] = (a_j x (tip - o_j)) . grad_path[r][t], a_j joint j's axis and o_j its origin in the base
 *   frame -- the position rows of avae_motion_pose's Jacobian contracted on the fly; the [rows][T][6][D] tensor is never formed.
 * avae_motion_eval_vjp: grad_params[r][d * Kb + k] = scale[d * Kb + k] sum_t phi[t][k] pass[r][t][d] grad_traj[r][t][d], pass = 1 where
 *   the unclamped q of avae_motion_eval satisfies lo_d <= q <= hi_d (everywhere without limits_dev, and for a joint whose hi <= lo);
 *   one fma chain over t per output.  The anchor term is constant in the parameters.
 * avae_rows_adam: P independent problems of n <= 1024 dimensions, one launch.  With cost_dev [P]: where cost < best_cost, x is
 *   copied into best_x and cost into best_cost first (x is where the cost was taken).  A row whose g holds a NaN or Inf then stays as
 *   it is (x, m, v, t) and gets status 2.  Otherwise g is scaled by min(1, max_norm / |g|_2) (max_norm <= 0: not at all), t = t + 1,
 *   m = beta1 m + (1 - beta1) g, v = beta2 v + (1 - beta2) g^2, x = x - lr (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps),
 *   status 0.
 * rows == 0 (P == 0) is a no-op.  Errors: as avae_stroke_render / avae_motion_fk / avae_motion_eval for the shared arguments; a NULL
 * required pointer; a cotangent or an output of img_l2 / height_l2 without target_dev / height_dev; n outside [1, 1024], lr < 0,
 * eps <= 0, beta outside [0, 1), cost_dev without best_cost_dev and best_x_dev.
 * One launch each, no floating-point atomics, no scratch, nothing of the handle is read or written: the calls work on any replica and
 * inside avae_use_averaged. */
int avae_stroke_render_vjp(avae_handle* h, const float* path_dev, int32_t rows, int32_t T, const float* plane_dev,
                           float half_width, float margin, int32_t H, int32_t ss,
                           const float* target_dev, const float* height_dev,
                           const float* g_image_dev, const float* g_img_l2_dev, const float* g_height_l2_dev,
                           float* grad_path_dev, float* image_dev, float* window_dev, float* img_l2_dev, float* height_l2_dev,
                           float* objective_dev, void* stream);
int avae_motion_fk_vjp(avae_handle* h, const float* traj_dev, int32_t rows, int32_t T, int32_t D,
                       const float* frames_dev, const float* axes_dev, const float* grad_path_dev, float* grad_traj_dev, void* stream);
int avae_motion_eval_vjp(avae_handle* h, const float* params_dev, int32_t rows, int32_t D, int32_t Kb, int32_t T,
                         const float* phi_dev, const float* scale_dev, const float* shift_dev, const float* limits_dev,
                         const float* anchor_gain_dev, const float* anchor_target_dev, int32_t nc,
                         const float* grad_traj_dev, float* grad_params_dev, void* stream);
int avae_rows_adam(avae_handle* h, float* x_dev, const float* g_dev, float* m_dev, float* v_dev, int32_t* t_dev, int32_t* status_dev,
                   int32_t P, int32_t n, float lr, float beta1, float beta2, float eps, float max_norm,
                   const float* cost_dev, float* best_cost_dev, float* best_x_dev, void* stream);

/* ---- letter thumbnails: from camera frames or drawing-pad canvases to the size x size pictures the image encoders were trained on
 * (DESIGN.md section 30).  The reference does this on the host for every input it is shown: the camera path thresholds the grey
 * frame at 108, inverts it and crops it to the ink (drawing_pad.py:185-193, writing_image_reader.py:64-97), the drawing pad converts
 * its RGBA canvas to grey and inverts it (drawing_pad.py:282-299, 311-322), and both -- like the data set (utils.py:46-107, 259-268)
 * -- hand the result to get_char_img_thumbnail_helper (utils.py:208-258): bounding box of the ink, pasted into a square canvas whose
 * side is the longer edge plus 60 %, cv2.resize(.., (28, 28), INTER_AREA).  This call is the project's own definition of that
 * picture, in integers throughout, so that its result is exact:
 *   frames_dev uint8 [rows][Hf][Wf][C], C = 1, 3 or 4; pixel (n, y, x) starts at byte n frame_stride + y row_stride + x C.  Bytes of
 *   a row behind Wf C and of a frame behind its last row are padding: never loaded.
 *   grey  v = the byte (C = 1), else (4899 R + 9617 G + 1868 B + 8192) >> 14; the bytes of a pixel are R, G, B (, A) or with
 *         AVAE_THUMB_BGR B, G, R (, A); the fourth byte is ignored.
 *   ink   threshold = -1 (none): g = 255 - v with AVAE_THUMB_INVERT, else v;  threshold in [0, 255]: t = v > threshold ? 255 : 0,
 *         g = 255 - t with AVAE_THUMB_INVERT, else t.  The camera path is threshold 108 with AVAE_THUMB_INVERT, the drawing pad no
 *         threshold with AVAE_THUMB_INVERT.
 *   box[n] = (x, y, w, h), the bounding box of the pixels with g != 0 (w, h counts of pixels), ink[n] their number.  A frame without
 *         ink is blank: box = (0, 0, Wf, Hf), ink = 0, every image pixel +0.
 *   window: L = max(w, h), b = 3 L / 5 (= int(0.6 L)), S = L + b, oy = b / 2 + (L - h) / 2, ox = b / 2 + (L - w) / 2 (integer
 *         divisions): frame pixel (y + r, x + c), r < h, c < w, is cell (oy + r, ox + c) of an S x S canvas of zeros.
 *         window[n] = (x - ox, y - oy, S): the canvas in frame coordinates.
 *   image[n][i size + j] = the mean of the canvas over [i S / size, (i + 1) S / size) x [j S / size, (j + 1) S / size), over 255:
 *         sum = sum over cells of g wy(i, row) wx(j, col),  wx(j, k) = max(0, min((j + 1) S, (k + 1) size) - max(j S, k size)), wy
 *         likewise -- an exact integer -- and image = (float)((double)sum / (double)(255 S S)), one division and one rounding.  The
 *         same rule holds for S < size (cv2.INTER_AREA interpolates there).
 * Differences from the reference: ink on the outermost pixels of the frame counts (cv2.findContours ignores it); the area mean is
 * kept for S < size; the grey value is the fixed-point formula above, not a bit copy of OpenCV's or PIL's; localize_img followed by
 * the helper is one pass (the second bounding box is the first one shifted).
 * avae_letter_thumbnail_plan (host only): slabs = the number of row bands a frame is scanned in (they tile Hf exactly, a function of
 *   Hf and Wf), workspace_bytes = what a call of `rows` frames needs.  Either output may be NULL, not both.
 * avae_letter_thumbnail: workspace_dev (16-byte aligned, at least the planned size, any contents: every byte read is written first
 *   by the same call).  Each of image_dev [rows][size size] float, box_dev [rows][4], window_dev [rows][3], ink_dev [rows] int32
 *   may be NULL, not all four.
 * rows == 0 is a no-op once the arguments have passed: it needs no workspace, but frames_dev and one output must still be non-NULL
 * (as avae_stroke_render asks).
 * Errors (message in avae_last_error, nothing launched): rows < 0 or > 2^24, Hf or Wf outside [1, 4096], C not 1, 3 or 4, size outside [1, 64], threshold outside [-1, 255], unknown flags, row_stride outside [Wf C, 2^26], frame_stride outside
 * [(Hf - 1) row_stride + Wf C, 2^38], frames_dev or workspace_dev NULL, every output NULL, a workspace below the plan or misaligned.
 * Two launches, no atomics, no scratch.  No model state is read or written -- of the handle the call takes the lock, the stream
 * bookkeeping and, in timing mode, the launch timers, as every entry point does: a frame's outputs are a pure function of its
 * bytes and the arguments -- the same alone or among other frames, on any stream, on repetition, with any workspace and whichever
 * outputs are asked for -- and the call works on any replica and inside avae_use_averaged. */
#define AVAE_THUMB_INVERT 1
#define AVAE_THUMB_BGR 2
int avae_letter_thumbnail_plan(int32_t rows, int32_t Hf, int32_t Wf, int32_t* slabs, size_t* workspace_bytes);
int avae_letter_thumbnail(avae_handle* h, const uint8_t* frames_dev, int32_t rows, int32_t Hf, int32_t Wf, int32_t C,
                          int64_t row_stride, int64_t frame_stride, int32_t flags, int32_t threshold, int32_t size,
                          void* workspace_dev, size_t workspace_bytes,
                          float* image_dev, int32_t* box_dev, int32_t* window_dev, int32_t* ink_dev, void* stream);

/* ---- pose, Jacobian and inverse kinematics: from a pen path back to joint angles.  The reference builds every
 * joint-modality row it trains on by solving one PyKDL inverse_kinematics per time point of a stroke, each seeded with the previous
 * point's solution (derive_ik_trajectory, baxter_writer.py:84-96), and returns from its Cartesian refinement to joint space the same
 * way (baxter_vae_assoc_writer.py:254).  These two calls are the project's own definition of what KDL's ChainIkSolverPos_NR over
 * ChainIkSolverVel_pinv does (baxter_pykdl_revised.py:165-204) -- damped least squares in place of a truncated-SVD pseudo-inverse --
 * not a bit copy of it.  Dense device fp32 everywhere but iterations_dev / status_dev (int32).  The chain is avae_motion_fk's
 * (frames_dev [D + 1][3][4], axes_dev [D][3]), walked from base to tip:  R_j, o_j the rotation and origin after F_j,  z_j = R_j axis_j.
 * avae_motion_pose: position[r][t] = the tip p, rotation[r][t] = the tip's rotation R (row-major 3 x 3), jacobian[r][t] the geometric
 *   Jacobian [6][D]:  J[0:3][j] = z_j x (p - o_j),  J[3:6][j] = z_j.  Each output may be NULL, not all three.  The position is the
 *   value of avae_motion_fk, not its bits: the chain is walked in the other direction.
 * avae_motion_ik: row r follows the T points path[r][:] from the angles seed[r][:].  Point 0 starts from the seed, point t from the
 *   angles point t - 1 ended with, whatever its status.  At a point, for k = 0, 1, ...:
 *     e_p = target - p;  with orient_dev (one goal R_g for every row, orient_rows = 1, or one per row, orient_rows = rows):
 *     e_w = 1/2 sum_i R[:, i] x R_g[:, i]  (sin(angle) times the axis: meant for goals within 90 degrees),  e = [e_p; e_w], m = 6;
 *     without a goal e = e_p, m = 3.   residual = |e_p|, rot_residual = |e_w| (NaN without a goal).
 *     status 0 (converged) when residual < tol and, with a goal, rot_residual < rot_tol -- strict, so tol = 0 never stops;
 *     status 1 (iteration cap) when k == n_iters;  else  M = J J^T + damping^2 I  over the m rows used,  M = L L^T (Cholesky; a
 *     pivot that is not > 0 ends the point with status 2),  dq = J^T M^-1 e,  scaled by max_step / max_j |dq_j| where that is below
 *     1,  q <- q + dq, clamped to limits_dev [D][2] when given.  A step is committed only when every new angle q_j + dq_j
 *     (after the scaling, before the clamp) is finite; otherwise none is stored and the point ends with status 2 as well.
 *   Status 2 is "the solve failed: a pivot not > 0 or a non-finite step" (a damping whose square underflows, a finite target so
 *   far away that M^-1 e overflows, about 1e36): the point keeps the last good q, the residuals at it and the steps taken so far,
 *   and the next point starts from that q.  With a finite seed no angle the call returns under status 0, 1 or 2 is NaN.
 *   traj[r][t] = the last q, residual / rot_residual those at that q (a pose evaluation: n_iters steps take n_iters + 1 of them),
 *   iterations the steps taken.  A non-finite target point gets NaN angles and residuals, 0 iterations and status 3 and leaves the
 *   carried angles alone (the next point behaves as if it had been deleted from the path); a non-finite seed does that to every
 *   point of its row.  Neither touches another row.  fp32 bottoms out near 2e-7 m on an arm of 1 m: a tol below about 1e-6 cannot
 *   be met.  csrc/avae_ik.h writes every operation and its order down.
 * rows == 0 is a no-op.  Errors (message in avae_last_error, nothing launched): rows < 0, D outside [1, 16], T outside [1, 1024],
 * n_iters outside [0, 1000], damping or max_step not > 0, tol or rot_tol negative or not finite, orient_rows neither 1 nor rows
 * (with orient_dev), a NULL required pointer (traj_dev of avae_motion_ik is required, its other outputs are optional), every
 * output of avae_motion_pose NULL.
 * One launch each, no atomics, no scratch, nothing of the handle is read or written: a row's outputs are a pure function of its
 * bits and the arguments -- the same alone or among other rows, on any stream, on repetition and whichever optional outputs are
 * asked for -- and the calls work on any replica and inside avae_use_averaged. */
int avae_motion_pose(avae_handle* h, const float* traj_dev, int32_t rows, int32_t T, int32_t D,
                     const float* frames_dev, const float* axes_dev,
                     float* position_dev, float* rotation_dev, float* jacobian_dev, void* stream);
int avae_motion_ik(avae_handle* h, const float* path_dev, int32_t rows, int32_t T, int32_t D,
                   const float* frames_dev, const float* axes_dev, const float* seed_dev,
                   const float* orient_dev, int32_t orient_rows, const float* limits_dev,
                   int32_t n_iters, float tol, float rot_tol, float damping, float max_step,
                   float* traj_dev, float* residual_dev, float* rot_residual_dev, int32_t* iterations_dev, int32_t* status_dev,
                   void* stream);

/* ---- joint-space inertia and inverse dynamics of the chain.  The reference takes inertia(q), coriolis(q, v) and
 * gravity(q) from KDL's ChainDynParam (baxter_dynamics, baxter_pykdl_revised.py:218-296) and prices a control u_t of its iLQR by
 * |M(q_t) u_t|^2 (baxter_writer.py:112-126).  This call is the project's own statement of the rigid-body dynamics of a serial chain
 * of revolute joints, for every (row, time point) at once, not a copy of KDL's.  Dense device fp32; gravity is a host vector.
 * The chain is avae_motion_pose's (frames_dev [D + 1][3][4], axes_dev [D][3]) with its walk:  o_j, z_j = R_j axis_j ahead of joint j's
 * rotation, R_j^+ behind it.  bodies_dev [D][10] holds per joint k (m, c[3], Ixx, Ixy, Ixz, Iyy, Iyz, Izz): mass, centre of mass
 * and inertia about it of everything that turns with joint k and not with joint k + 1, in the frame behind joint k's rotation
 * (KinematicChain.bodies); a mass of 0 is allowed.  With r_k = R_k^+ c_k and I_k^w = R_k^+ I_k R_k^+T, by value:
 *     M(q)    = sum_k [ m_k Jv_k^T Jv_k + Jw_k^T I_k^w Jw_k ],   Jv_k[:, j] = z_j x (o_k + r_k - o_j),  Jw_k[:, j] = z_j  (j <= k, else 0)
 *     g(q)    = dV/dq,   V = -sum_k m_k grav . (o_k + r_k)
 *     c(q, v) = the Christoffel terms of M:  c_i = sum_jk (dM_ij/dq_k - 1/2 dM_jk/dq_i) v_j v_k
 *     tau     = M a + c + g
 *   traj / vel / acc are [rows][T][D]; vel_dev NULL means v = 0, acc_dev NULL a = 0.  inertia[r][t] = M [D][D], symmetric bit for bit;
 *   gravity[r][t] = g [D];  coriolis[r][t] = c [D] (the torque at a = 0 and grav = 0);  torque[r][t] = M a + c + g [D].  Each output
 *   may be NULL, not all four.  With vel_dev NULL and gravity = 0, torque is the reference's M(q_t) u_t for acc = u.
 *   As computed: recursive Newton-Euler in base-frame coordinates, one pass per output and D unit-acceleration passes for M (the
 *   upper triangle of each column kept and mirrored); csrc/avae_dynamics.h writes every operation and its order down.  A point with
 *   a non-finite angle, speed or acceleration has NaN in all its outputs and touches no other point.
 * rows == 0 is a no-op.  Errors (message in avae_last_error, nothing launched): rows < 0, D outside [1, 16], T outside [1, 1024], a
 * non-finite gravity, a NULL required pointer (traj_dev, frames_dev, axes_dev, bodies_dev, gravity), every output NULL.
 * One launch, no atomics, no scratch, nothing of the handle is read or written: a point's outputs are a pure function of its bits and
 * the arguments -- the same alone or among other points, on any stream, on repetition and whichever outputs are asked for -- and the
 * call works on any replica and inside avae_use_averaged. */
int avae_motion_dynamics(avae_handle* h, const float* traj_dev, const float* vel_dev, const float* acc_dev,
                         int32_t rows, int32_t T, int32_t D, const float* frames_dev, const float* axes_dev,
                         const float* bodies_dev, const float* gravity,
                         float* inertia_dev, float* gravity_dev, float* coriolis_dev, float* torque_dev, void* stream);

/* ---- sigma-lognormal strokes: batched evaluation, perturbed sampling and fitting on the device.  The
 * reference diversifies its handwriting data by fitting every letter with a sum of lognormal velocity components
 * (pytrajkin_rxzero.rxzero_train), perturbing each component's amplitude, start angle and straightness and evaluating the stroke
 * again (extend_data_with_lognormal_sampling, utils.py:311-359; the model: pytrajkin_rxzero.py:241-292, 356-388).  These calls are
 * the project's own statement of that model and a Levenberg-Marquardt fit of it, not a bit copy of the reference's optimiser.
 * Dense device fp32 everywhere but count_dev / iterations_dev / accepted_dev / status_dev (int32), loss0_dev / loss_dev (double) and
 * free_dev (uint8).  A stroke of row r is count[r] components p_c = (D, t0, mu, sigma, theta_s, theta_e) out of params[r][C][6]
 * (count_dev NULL: all C; components c >= count[r] are never read; a count[r] outside [0, C] is read as clamped into it, in all
 * three calls), evaluated at t_k = k dt, k < T, from start[r] = (x0, y0):
 *     tau = t_k - t0,  sg = max(sigma, 1e-6),  on = tau >= 1e-6,  tc = max(tau, 1e-6),  z = (ln tc - mu) / sg
 *     amp = on ? D exp(-z^2 / 2) / (sg sqrt(2 pi) (tc + 1e-5)) : 0,   phi = theta_s + (theta_e - theta_s) / 2 (1 + erf z)
 *     v_k = sum_c |amp| (cos phi, sin phi)  (c ascending),   path_k = start + dt sum_(j <= k) v_j  (inclusive)
 *   in fp32, with ln, exp, erf, sin and cos taken in double on the float argument and rounded once (the correctly rounded float
 *   result: the bits do not depend on a math library's choice within its ulp).
 * avae_lognormal_eval: path[r][k] and, unless NULL, velocity[r][k] = v_k.  A row with a non-finite start or parameter (c < count)
 *   is NaN everywhere and touches no other row.
 * avae_lognormal_sample: for row r, sample s and component c one Philox4x32-10 block of the library's stream,
 *     counter = (row_offset + r, s, c, 0),  key = (seed lo, seed hi ^ 0x736c676e 'slgn'),
 *   whose first three Box-Muller normals divided by 3 are (n0, n1, n2);  D' = D + n0 amplitude D,  theta_s' = theta_s + n1 angle,
 *   theta_e' = theta_e + n1 angle + n2 straightness (theta_e - theta_s), the rest unchanged.  strokes[r][s] is what
 *   avae_lognormal_eval gives for those parameters, bit for bit; with shift_mean the sample's own mean point is subtracted.
 *   perturbed[r][s][c] (may be NULL) are the perturbed components, zeros for c >= count[r].  Nothing of size rows * S * C * 6 is
 *   stored otherwise.  The handle's draw counter is neither read nor advanced: a caller who samples rows in chunks passes each
 *   chunk's first row as row_offset and gets the bits of the whole.
 * avae_lognormal_fit: fits count[r] components to target[r][T][2] from init[r][C][6], the whole loop of a row inside one launch.
 *     V_0 = (P_0 - start) / dt,  V_k = (P_k - P_(k-1)) / dt;   the loss  L = wp sum |path - P|^2 + wv sum |v - V|^2;
 *     model values and Jacobian entries are fp32;  M = J^T W J, g = J^T W e and L are accumulated in double.
 *     free_dev (NULL: every parameter free; [6], free_per_row 0; or [rows][C][6], free_per_row 1; nonzero = free) takes parameters
 *     out: their rows and columns of M are 0 with a 1 on the diagonal, and 0 in g.  With d = diag(M) of the free parameters:
 *     M += diag(lam d + 1e-12 (max d + 1));  a Cholesky in double (a pivot not > 0, or a non-finite solution, rejects the step);
 *     new = p - M^-1 g rounded to float, sigma clipped into [1e-3, 3], then into [lo_dev[j], hi_dev[j]] (each [6] or NULL);
 *     L(new) < L accepts: lam = max(lam / 3, 1e-9), and the row ends with status 0 when L - L(new) < tol L;
 *     else lam = min(4 lam, 1e9) and p stays.  lam starts at 1e-3.
 *     8 rejected tries in a row end the row as well: the damping has grown 65536-fold and nothing lowers the loss, which is how every
 *     fit ends that reaches the floor of fp32 (a loss near 1e-12 on strokes of extent 1) -- status 0 when a step was accepted
 *     before them, status 2 (the row cannot improve) when none ever was.
 *   status: 0 converged, 1 n_iters tries made, 2 no step accepted at all in 8 tries, 3 a non-finite target, start or initial
 *   parameter (c < count): that row's params, loss0 and loss are NaN, 0 iterations, and nothing else is touched.  count 0: nothing
 *   to fit, 0 iterations, status 0, loss = loss0 that of standing still.  params[r][c] = 0 for c >= count[r].  loss0 the loss at
 *   init, iterations the tries made, accepted the steps taken.  Every output but params_dev may be NULL.
 *   csrc/avae_lognormal.h writes every operation and the order of every sum down.
 * rows == 0 is a no-op.  Errors (message in avae_last_error, nothing launched): rows < 0, C outside [1, 16], T outside [1, 1024],
 * dt not > 0, S outside [1, 2^20] or rows * S >= 2^31, row_offset < 0 or row_offset + rows > 2^32, amplitude, angle, straightness,
 * wp, wv or tol negative or not finite, n_iters outside [0, 10000], a NULL required pointer.
 * One launch each, no atomics, no scratch, nothing of the handle is read or written: a row's outputs are a pure function of its
 * bits and the arguments -- the same alone or among other rows, on any stream, on repetition and whichever optional outputs are
 * asked for -- and the calls work on any replica and inside avae_use_averaged. */
int avae_lognormal_eval(avae_handle* h, const float* params_dev, const int32_t* count_dev, const float* start_dev,
                        int32_t rows, int32_t C, int32_t T, float dt, float* path_dev, float* velocity_dev, void* stream);
int avae_lognormal_sample(avae_handle* h, const float* params_dev, const int32_t* count_dev, const float* start_dev,
                          int32_t rows, int32_t S, int32_t C, int32_t T, float dt, uint64_t seed, int64_t row_offset,
                          float amplitude, float angle, float straightness, int32_t shift_mean,
                          float* strokes_dev, float* perturbed_dev, void* stream);
int avae_lognormal_fit(avae_handle* h, const float* target_dev, const float* init_dev, const int32_t* count_dev,
                       const float* start_dev, int32_t rows, int32_t C, int32_t T, float dt, int32_t n_iters,
                       double wp, double wv, double tol, const uint8_t* free_dev, int32_t free_per_row,
                       const float* lo_dev, const float* hi_dev,
                       float* params_dev, double* loss0_dev, double* loss_dev, int32_t* iterations_dev, int32_t* accepted_dev,
                       int32_t* status_dev, void* stream);

/* ---- joint-trajectory synthesis: batched iLQR on a double-integrator joint model.  The reference builds its
 * smooth joint-modality rows by taking the point-by-point IK solution as a first guess and running 25 iLQR iterations that trade
 * Cartesian tracking against control effort (BaxterWriter.derive_ilqr_trajectory, baxter_writer.py:106-145).  This call is the
 * project's own statement of that solver -- Gauss-Newton linearisation of the tracking cost, a Riccati recursion regularised on the
 * control, full steps accepted or rejected by the cost -- not a bit copy of it.  Dense device fp32 everywhere but cost0_dev /
 * cost_dev (double) and iterations_dev / accepted_dev / status_dev (int32).  The chain is avae_motion_fk's; p(q) is the tip of
 * avae_motion_pose's walk, J_v the linear rows of its Jacobian.
 *   Row r has states x_t = (q_t, v_t), t < T, and controls u_t, t < T - 1:  q_(t+1) = q_t + dt v_t,  v_(t+1) = v_t + dt u_t,
 *   x_0 = (init[r][0], 0).  The first controls:  v0_0 = 0,  v0_t = (init_t - init_(t-1)) / dt,  u_t = (v0_(t+1) - v0_t) / dt.
 *   The cost  J = sum_t |w (p(q_t) - path_t)|^2 + sum_(t < T-1) u_t^T S u_t + wl sum_t sum_j max(0, q_tj - hi_j, lo_j - q_tj)^2,
 *   w = track_w[3] (host memory),  S = R E^T E with effort_dev = E [D][D], S = R I with NULL;  the limit term only with
 *   limits_dev [D][2] and limit_weight = wl > 0.
 *   A try at the damping lam:  l_q = 2 J_v^T w^2 e (+ 2 wl viol),  l_qq = 2 J_v^T w^2 J_v (+ 2 wl on violated diagonals),
 *   l_u = 2 S u,  l_uu = 2 S (no second derivatives of the kinematics);  backwards from V_x = l_x(T-1), V_xx = l_xx(T-1):
 *     Q_x = l_x + A^T V_x,  Q_u = l_u + B^T V_x,  Q_xx = l_xx + A^T V_xx A,  Q_ux = B^T V_xx A,  Q_uu = l_uu + B^T V_xx B + lam I,
 *     k = -Q_uu^-1 Q_u,  K = -Q_uu^-1 Q_ux  (Cholesky; a pivot not > 0 or a non-finite gain rejects the try without a rollout),
 *     V_x = Q_x + K^T Q_uu k + K^T Q_u + Q_ux^T k,   V_xx = Q_xx + K^T Q_uu K + K^T Q_ux + Q_ux^T K, symmetrised;
 *   forwards  u'_t = u_t + k_t + K_t (x'_t - x_t), a full step.  J' < J accepts the try: lam = max(lam / factor, lam_min), and the
 *   row ends with status 0 when J - J' < tol J (strict: tol = 0 never stops).  Otherwise lam = lam factor and the trajectory
 *   stays; the row ends when lam > lam_max, with status 0 if a try was ever accepted and status 2 if none was.  Status 1: n_iters
 *   tries made.  T = 1: no controls, traj = init[0], 0 tries, status 0, cost = cost0.  Status 3: a non-finite path point, init
 *   value or (used) limit: that row's traj, controls, cost0, cost and track_rmse are NaN, 0 tries, and nothing else is touched.
 *   The walk, the Jacobian, l_q and l_qq are fp32 in avae_motion_pose's order (its sines and cosines taken in double on the
 *   float angle and rounded once, so that the bits do not depend on a math library's choice within its ulp); J, the whole value
 *   recursion, the Cholesky, the gains' formation and the rollout are double; the stored gains, traj and controls are rounded
 *   once to float.  csrc/avae_track.h writes every operation and the order of every sum down.
 *   Outputs: traj [rows][T][D] (required); controls [rows][T-1][D], cost0 (J of the first trajectory), cost, track_rmse
 *   (sqrt(mean_t |p(q_t) - path_t|^2) of the returned trajectory), iterations (tries made), accepted, status: each may be NULL.
 *   workspace_dev (8-byte aligned) holds the gains and the row's trajectories: avae_motion_track_plan gives its size,
 *   rows * roundup(T (10 D^2 + 58 D), 256) bytes (host only, no handle, works without a GPU; its message goes to
 *   avae_last_error(NULL)).  Its contents after the call are unspecified.
 * rows == 0 is a no-op.  Errors (message in avae_last_error, nothing launched): rows < 0, D outside [1, 16], T outside [1, 1024],
 * dt, factor - 1, lam0 or lam_min not > 0, lam_max < lam0, a track weight, R, limit_weight or tol negative or not finite, n_iters
 * outside [0, 1000], workspace_bytes below the plan's, a NULL required pointer.
 * One launch, no atomics, no scratch memory, nothing of the handle is read or written: a row's outputs are a pure function of its
 * bits and the arguments -- the same alone or among other rows, on any stream, on repetition, whichever optional outputs are asked
 * for and however large the workspace -- and the call works on any replica and inside avae_use_averaged. */
int avae_motion_track_plan(int32_t rows, int32_t T, int32_t D, size_t* workspace_bytes);
int avae_motion_track(avae_handle* h, const float* path_dev, const float* init_dev, int32_t rows, int32_t T, int32_t D,
                      const float* frames_dev, const float* axes_dev, float dt, const float* track_w, float R,
                      const float* effort_dev, const float* limits_dev, float limit_weight,
                      int32_t n_iters, double lam0, double factor, double lam_min, double lam_max, double tol,
                      void* workspace_dev, size_t workspace_bytes,
                      float* traj_dev, float* controls_dev, double* cost0_dev, double* cost_dev, float* track_rmse_dev,
                      int32_t* iterations_dev, int32_t* accepted_dev, int32_t* status_dev, void* stream);

/* ---- black-box search around a cost: batched PI-BB / CEM iterations on the device.  The reference refines a
 * predicted motion by drawing rollouts from a Gaussian, pricing each and refitting the Gaussian to the cost-weighted rollouts
 * (pygcem.py:28-151, driven from baxter_vae_assoc_writer.py:259-342).  Here P such searches ("problems") advance at once: problem p
 * owns N(mean[p], diag(var[p])) over n dimensions and draws R rollouts per iteration; the caller prices x [P][R][n] into cost [P][R]
 * between the two calls.  Dense device fp32 everywhere but n_applied_dev / frozen_dev (int32).
 * avae_search_sample: x[p][r][d] = fma(sqrtf(var[p][d]), N, mean[p][d]), N the Box-Muller normal of the library's eps stream
 *   (Philox4x32-10, the block's four normals to four consecutive dimensions) under a key of the call's own:
 *     counter = (problem_offset + p, r, d / 4, iteration),  key = (seed lo, seed hi ^ 0x73726368 'srch').
 *   The key is the call's seed, not the handle's, and the handle's draw counter is neither read nor advanced: the stream depends on
 *   nothing else the handle did, and a caller who prices P problems in chunks passes each chunk's first problem as problem_offset
 *   and gets the bits of the whole.  With proj_A_dev [G][g][g] and proj_b_dev [P][n] (G * g == n, g <= 64; both or neither) group
 *   k of g consecutive dimensions is mapped  x_k <- A_k x_k + b[p]_k,  element j as  acc = b; acc = fma(A[j][i], x[i], acc), i
 *   ascending -- what gaussian_sampling does under a linear constraint (pyrbf_funcapprox.py:163-171); the kernel knows nothing of
 *   constraints, vae_assoc_amd/motion.py folds them into (A, b).
 * avae_search_update: one GaussianCEM.fit per problem over the rollouts with a finite cost (a NaN or Inf cost, which is how a
 *   motion that cannot be drawn is priced, has weight 0 and enters no statistic), in IEEE double, rounded once into the outputs:
 *     weights   PI-BB : w = exp(-eliteness (c - min) / (max - min + 1e-6));  CEM: the mu = eliteness lowest costs get 1 / mu, ties
 *               to the lower rollout;  CMA-ES: those get log(mu + 1/2) - log(rank + 1);  all 1 where std(c) <= 1e-8 |mean(c)|
 *               (population std); then w / sum w
 *     mean'     = sum_r w_r x_r
 *     var'      = (1 - lr) var + lr sum_r w_r (x_r - m)^2,  m the old mean (cov_update PI-BB) or mean' (CEM); diagonal only
 *     bounds    (each off when negative) var' = min(var', abs_upper); then var' = max(var', max(abs_lower, rel_lower max_d var'))
 *     moved     = |mean' - mean|_2;  moved < tol sets frozen[p]: from the next call on the problem is left alone (tol 0: never)
 *   A problem with no finite cost, or frozen on entry, keeps mean, var and n_applied bit for bit and gets NaN in avg_cost, min_cost
 *   and moved; else n_applied[p] += 1, avg_cost / min_cost = the mean / minimum of the finite costs.  best_cost / best_x keep the
 *   lowest finite cost over every rollout the calls saw and its x (a later equal cost does not replace it; start best_cost at +inf).
 *   avg_cost_dev, min_cost_dev, moved_dev may be NULL.  csrc/avae_search.h writes every operation and the order of every sum down.
 * P == 0 is a no-op.  Errors (message in avae_last_error, nothing launched): P < 0, n or R outside [1, 1024], iteration < 0,
 * problem_offset < 0 or problem_offset + P > 2^32, one of proj_A / proj_b without the other, G * g != n, g outside [1, 64], an
 * unknown weighting or cov_update, eliteness not finite and >= 0 (CEM / CMA-ES: not a whole number >= 1), learning_rate outside
 * [0, 1], rel_lower > 1, a bound or tol that is NaN or infinite, tol < 0, a NULL required pointer.
 * One launch each, no atomics, no scratch, one fixed order of every sum, nothing of the handle is read or written: a problem's
 * outputs are a pure function of its own bits and the options -- the same alone or among other problems, on any stream, on
 * repetition and whichever optional outputs are asked for -- and the calls work on any replica and inside avae_use_averaged. */
#define AVAE_SEARCH_PIBB 0
#define AVAE_SEARCH_CEM 1
#define AVAE_SEARCH_CMAES 2
typedef struct avae_search_options {
    int32_t weighting;          /* AVAE_SEARCH_PIBB, _CEM or _CMAES */
    int32_t cov_update;         /* AVAE_SEARCH_PIBB (deviations from the old mean) or AVAE_SEARCH_CEM (from the new one) */
    double eliteness;           /* PI-BB: h;  CEM / CMA-ES: mu */
    double learning_rate;
    double rel_lower, abs_lower, abs_upper;   /* variance bounds; negative: off */
    double tol;
} avae_search_options;
int avae_search_sample(avae_handle* h, const float* mean_dev, const float* var_dev, int32_t P, int32_t R, int32_t n,
                       uint64_t seed, int32_t iteration, int64_t problem_offset,
                       const float* proj_A_dev, const float* proj_b_dev, int32_t G, int32_t g, float* x_dev, void* stream);
int avae_search_update(avae_handle* h, const float* x_dev, const float* cost_dev, int32_t P, int32_t R, int32_t n,
                       const avae_search_options* opt,
                       float* mean_dev, float* var_dev, int32_t* n_applied_dev, int32_t* frozen_dev,
                       float* best_cost_dev, float* best_x_dev,
                       float* avg_cost_dev, float* min_cost_dev, float* moved_dev, void* stream);

/* save_model / restore_model (vae_assoc.py:427-463): own flat file (config echo + params + Adam
 * slots + step; with parameter averaging on also its settings and the average, see avae_set_ema);
 * TF .ckpt files cannot be read offline. */
int avae_save(avae_handle* h, const char* path);
int avae_load(avae_handle* h, const char* path);

/* ---- AVAE_INTROSPECTION: bench.py / tests only; no caller of the reference's surface needs anything below ---- */
int avae_synchronize(avae_handle* h);
/* Average device time (ms) of every launch of the step over the calls since the last reset,
 * measured with hipEvents on the stream the kernels were launched on (hipExtLaunchKernel start/stop
 * events: the dispatch's own begin and end, what rocprofv3 --kernel-trace reports).  Only recorded
 * while timing is enabled (it forces eager launches instead of graph replay); "_null_kernel" is a
 * one-store kernel timed the same way.  Report: one line "<name> <calls> <avg_ms> <min_ms>" per launch. */
int avae_timing_enable(avae_handle* h, int32_t on);
int avae_timing_report(avae_handle* h, char* buf, size_t buf_bytes);
/* The gradient collective of bucket `bucket` alone, on `stream` (micro-benchmarks and tests of the exchange; the train calls run it
 * on the library's comm stream inside the step).  Every rank must make the same sequence of calls. */
int avae_comm_allreduce(avae_handle* h, int32_t bucket, void* stream);
/* Copies a named internal tensor to the host as fp32 (tests): "mulv<m>" [batch,2*n_z], "eps" [batch,n_z], "E<m>_<k>" / "D<m>_<k>" the
 * stored output of encoder / decoder hidden layer k of modality m [batch, width] (the last forward pass's relu decisions);
 * "shadow_err" -> {max |W - theta|, max |W^T - theta|, layers checked, worst layer}: the compute-dtype weight shadows against the
 * parameters rounded once (must be 0, 0 after any call); "X<m>" staging set 0's encoder input of modality m [batch, n_input] (the
 * compute-dtype copy, widened), "T<m>" its exact loss target; "ema_master" the parameter average as it lies in memory (the internal
 * padded layout, padding included).  While avae_use_averaged is on, "shadow_err" compares against the average.
 * "grad_keep" (the plain plan; "grad_keep_masked": the masked one) -> per captured step of the plan's training graphs, the 16-step
 * graph's first, then the 4-step graph's, then the single step's (21 values): 1 = that step stores its gradient. */
int avae_debug_fetch(avae_handle* h, const char* name, float* host_dst, size_t max_floats, size_t* n_floats);

#ifdef __cplusplus
}
#endif
#endif /* AVAE_H_ */
