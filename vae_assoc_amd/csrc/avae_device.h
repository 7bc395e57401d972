// Device-visible descriptors shared by the host planner (avae_host.hip) and the gfx950 kernels
// (avae_kernels.hip).  A training step is a fixed list of launches; each launch runs ONE
// grouped kernel over a table of work items passed by value in its kernel arguments; nothing in it
// changes after avae_create, which is what lets the whole step be captured once as a hipGraph.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stdint.h>
#include "../../include/avae.h"

namespace avae {

constexpr int kMaxMod = 4;
constexpr int kThreads = 256;          // 4 wavefronts of 64
constexpr int kTileBytesK = 128;       // bytes of K per staged tile row: 64 bf16 or 32 f32
constexpr int kRowAlign = 256;         // row counts of GEMM operands are padded to this (largest tile)
constexpr int kLatentRows = 16;        // rows per latent work-item tile (many small blocks: the item is latency-bound)
constexpr int kAdamRows = 16;          // k_adam tiles are kAdamRows x 64: measured 64 -> 32 -> 16 rows = 10.3 -> 9.8 -> 9.2 us on C2 (more,
                                       // lighter workgroups balance better over 256 CUs and overlap each other's load and store
                                       // phases); 8 rows (128 threads) 9.3 us and 16-byte segments in the transposed shadow
constexpr int kCostHist = 4096;        // ring of per-step costs kept on the device
// k_grad_sumsq (global-norm clipping): G = sumsq_blocks(P_int) workgroups of kSumsqThreads threads.  A thread owns the 16-byte quads
// tid + k * G * kSumsqThreads of the gradient buffer (k = 0, 1, ...: sumsq_chain(P_int) of them at most) and keeps one accumulator per
// quad element.  G depends on P_int alone -- never on the device -- so the order of the sum is a constant of the model.
constexpr int kSumsqThreads = 256;
constexpr int kSumsqMaxBlocks = 256;   // G <= 256: k_adam's wave 0 sums the partials, four per lane
constexpr int kSumsqQuads = 8;         // quads per thread below which G grows instead of the chain (128 B in flight per lane)
inline int sumsq_blocks(long long p_int) {
    const long long quads = p_int / 4, per_block = (long long)kSumsqThreads * kSumsqQuads;
    const long long g = (quads + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : g > kSumsqMaxBlocks ? kSumsqMaxBlocks : g);
}
inline int sumsq_chain(long long p_int) {
    const long long quads = p_int / 4, per_pass = (long long)kSumsqThreads * sumsq_blocks(p_int);
    return (int)((quads + per_pass - 1) / per_pass);
}

// Work-item kinds.  Forward / dgrad kinds compute C[M,N] = sum_k A[m][k] * B[n][k] ("NT": both operands K-contiguous),
// K_WGRAD computes C[M,N] = sum_k A[k][m] * B[k][n] ("TN": both operands as stored, K = batch); they differ otherwise
// only in the LDS-staged epilogue.  Every result is stored once, row-major.
enum Kind : int {
    K_FWD_HIDDEN = 0,    // Y = act(X_aug . W_aug)                      -> Y               (vae_assoc.py:187,203,259,282)
    K_FWD_HEAD = 1,      // [mu|lv] = H_aug . Whead_aug; z = mu+exp(lv/2)*eps -> mulv, Z   (:217-221,:102-103)
    K_FWD_OUT_LOSS = 2,  // logits; recon loss + dLoss/dlogits         -> dA, cost partial (:293-303,:321-328)
    K_FWD_OUT_STORE = 3, // x_hat = sigmoid(logits) | logits           -> fp32 (inference)
    K_DGRAD_HIDDEN = 4,  // dA_prev = (dA . W^T) * act'(Y_prev)        -> dA_prev
    K_DGRAD_LATENT = 5,  // dz = dA . V1^T; dmu, dlv via reparam + static latent grads -> dH
    K_WGRAD = 6,         // dW_aug = X_aug^T . dA (bias grad = last row) -> fp32 gradient
    K_DGRAD_F32 = 10,    // dP = dA . W^T stored as fp32 (conv branch: patch gradients, summed by k_col2im)
    K_LATENT = 7,        // KL(q||N(0,I)) + association penalty: cost partials + static (mu,lv) grads (:335-366)
    K_COST = 8,          // fixed-order sum of the cost partials -> grad[cost slot]; bumps the step counter
    K_SERVE_Z = 11,      // serving (avae_generate): no product of its own (K = 0) -- the call's fp32 z rows (aux0, n_slots rows, dense
                         // [rows][nz]) go into the 32x64 tile's LDS image and the tail product (tail_*) is the decoder's first
                         // layer; workgroup 0 publishes the call's slot (partial = ServeSlot*, out0/out1/out2/aux1 = the call's
                         // output pointers of modality 0..3).  Launched per call with these fields patched by value.
};

// What a launch of a plan runs (host: Launch::type) and, for the grouped GEMM launches, on which tile configuration (Launch::cfg).
// The values are pinned: the plan dumps print them as integers ("type=%d cfg=%d"), and tests/plan_dump.py, the tests' cfg
// assertions and the logs under profiles/ read those numbers.
enum LaunchType : int {
    kGrouped = 0,        // a grouped GEMM kernel (k_grouped, the k_small family) on Launch::cfg
    kGather = 1,         // k_gather (im2col)
    kCol2im = 2,         // k_col2im
    kReduce = 3,         // k_reduce (split-K slices -> gradient)
    kThin = 4,           // k_thin (the direct one-channel stage)
    kColsum = 5,         // k_colsum
    kWadj = 6,           // k_wadj
    kGperm = 7,          // k_gperm
    kRowsum = 8,         // k_rowsum
    kSums = 9,           // k_sums (column sums + slice sums in one launch)
};
enum TileCfg : int {
    k64x64 = 0,          // 4-stage ring
    k128x128 = 1,        // 2-stage ring, two workgroups per CU
    k256x128 = 2,        // 8 waves, 3-stage ring, one workgroup per CU (big single-C-tile kinds only)
    k32x64 = 3,          // NT launches with too few 64x64 tiles to occupy the chip
    k64x128 = 4,         // wide-latent head / latent-dgrad launches with few tiles
    k32x32 = 5,          // as k32x64, for launches without head kinds
    k256x64Loss = 6,     // 8 waves, register epilogue: the output + loss launch of the big nets
    kLean = 7,           // k_small: one kind and one transfer function per launch
                         // (8 is unused: a closed experiment's number, kept free so that old logs stay readable)
    kLeanLoss = 9,       // k_small_loss: output + loss, the latent item riding along
    kLeanLatb = 10,      // k_small_latb: bwd_dec1_latent + bwd_head
    kLeanHead = 11,      // k_small_head: fwd_head + fwd_dec1
    kLeanTnAdam = 12,    // k_small_tn: every weight gradient with Adam in the epilogue
    kChain2 = 13,        // k_chain2 (AVAE_CHAIN2)
};
// The one table of tile geometry: tile rows x columns, threads of a workgroup (NT instance), stages of the operand ring, and what
// the kernel behind the configuration can do.
struct TileGeom {
    int rows, cols, threads, ring;
    bool waves8;         // the 8-wave tiles: bias epilogue, weight warm-up, one workgroup per CU
    bool lean;           // a kernel of the k_small family (its own LDS frame)
    bool gather;         // carries the implicit-GEMM gather (WorkItem::conv)
    bool masked;         // has an instance with the presence gate (WorkItem::present)
    int records;         // lines of a per-workgroup record the training plan may run it on (0: by-value arguments only)
};
constexpr int kTileCfgs = 14;
constexpr TileGeom kTileGeom[kTileCfgs] = {
    {64, 64, 256, 4, false, false, true, true, 0},        // k64x64
    {128, 128, 256, 2, false, false, false, true, 0},     // k128x128
    {256, 128, 512, 3, true, false, false, false, 0},     // k256x128
    {32, 64, 256, 4, false, false, true, true, 0},        // k32x64
    {64, 128, 256, 4, false, false, false, true, 0},      // k64x128
    {32, 32, 256, 4, false, false, true, true, 0},        // k32x32
    {256, 64, 512, 3, true, false, false, true, 0},       // k256x64Loss
    {32, 32, 256, 4, false, true, false, false, 1},       // kLean
    {0, 0, 0, 0, false, false, false, false, 0},          // (unused)
    {32, 32, 256, 4, false, true, false, true, 2},        // kLeanLoss
    {32, 64, 256, 4, false, true, false, false, 2},       // kLeanLatb
    {32, 64, 256, 4, false, true, false, false, 2},       // kLeanHead
    {64, 64, 256, 4, false, true, false, false, 1},       // kLeanTnAdam
    {32, 32, 256, 4, false, true, false, false, 0},       // kChain2
};
constexpr const TileGeom& tile_geom(int cfg) { return kTileGeom[cfg]; }
constexpr int tile_ring_bytes(int cfg) { return kTileGeom[cfg].ring * (kTileGeom[cfg].rows + kTileGeom[cfg].cols) * kTileBytesK; }

struct WorkItem {
    int kind;
    int M, N, K;             // K is the padded extent (multiple of the K unit)
    int lda, ldb;            // in elements of the compute type
    int tiles_m, tiles_n;
    int act;                 // AVAE_ACT_*
    int ld0, ld1, ldx;
    int nz;
    int binary;
    int ksplit, kchunk;      // K_WGRAD with a long K (conv stages: K = batch x output pixels): the K range is cut into ksplit
                             // chunks of kchunk K tiles, chunk s writing its own fp32 slice out1 + s*M*ld0 (summed by k_reduce)
    int bias_row;            // K_WGRAD, > 0: the tiles cover rows [0, M) = the weight rows only and the bias gradient (row
                             // bias_row = M, the column sums of dA) comes from one extra MFMA per fragment with an all-ones A
                             // operand in the first tile row -- set by the host when M+1 rows would cost a whole tile row more
    int bias_ep;             // forward kinds on the 8-wave tiles, set by the host when fan-in % K-unit == 0: K stops at the fan-in
                             // (the bias row would cost a whole K tile more) and the epilogue adds bias[n] = aux1[n] instead
    int kin;                 // forward kinds: fan-in of the layer (the bias is row kin of W_aug)
    int tile_off, tile_cnt;  // K_WGRAD launches only (TnItem)
    int slot_base;           // first cost-partial slot written by this item
    int n_slots;             // K_COST: number of partial slots to sum
    int n_mod;               // K_LATENT
    int bump_step;           // K_COST: 1 in training graphs
    float scale;             // w/B_global (mean terms) or w (sum terms)
    float lambda;            // K_LATENT
    float inv_bg;            // 1/B_global
    const void* A;
    const void* B;
    void* out0;
    void* out1;
    void* out2;
    const void* aux0;
    const void* aux1;
    const void* aux2;
    float* partial;          // cost partial slots
    const float* eps;        // K_LATENT: the step's eps [B][ldx]
    float wts[kMaxMod];      // K_LATENT: per-modality cost weights
    // Tail product (small nets, 32x64 head tiles): K_FWD_HEAD / K_DGRAD_LATENT items leave a narrow result (z, or [dmu | dlv]) whose
    // only consumer is a layer that multiplies over one or two K tiles (the decoder's first layer, K = n_z + 1; the heads' input
    // gradient, K = 2 n_z) and used to be a launch of its own.  With tail_mode set the same workgroup multiplies its 32 result rows, still in
    // LDS, with that layer's weight shadow (B fragments straight from global memory into registers) and stores the layer's
    // output: forward  out = act(z_aug . W^T),  dgrad  out = ([dmu|dlv] . W^T) * act'(aux).  The item's tiles_n then counts tail
    // SLICES of 64 output columns: slice s of a row block is a workgroup of its own that recomputes the 32x64 head tile (cheap: the
    // slices of a row block share an XCD and its L2) and multiplies columns [64 s, 64 s + 64); slice 0 also stores the head's results.
    const void* tail_w;      // [tail_n][tail_ldw]: K-contiguous weight shadow of the consuming layer
    void* tail_out;          // [rows][tail_ldo]
    const void* tail_aux;    // mode 2: stored output of the layer the gradient belongs to [rows][tail_ldx]
    int tail_mode;           // 0: none; 1: forward hidden layer; 2: dgrad of a hidden layer
    int tail_n;              // units of the consuming layer (columns of its output)
    int tail_ldw, tail_ldo, tail_ldx;
    int tail_act;
    int tail_kt;             // K tiles of the consuming layer's product: 1, or 2 (fp32 [dmu | dlv] with n_z > 16)
    int conv;                // > 0: the A operand is an implicit patch matrix, descriptor conv - 1 of the launch's ConvA table (below)
    // Masked steps (avae_train_steps_masked / avae_eval_cost_masked): the staged presence bytes of the batch, row n at
    // present[n * present_ld] -- K_FWD_OUT_LOSS: already at the item's modality column; K_LATENT: modality m at + m.
    // Nonzero = observed.  Null in every unmasked plan: the loss and latent sites then take no presence test at all.
    const unsigned char* present;
    int present_ld;
    // K_LATENT reuses the pointer fields: [mu|lv] inputs of modality 0..3 = A, B, aux0, aux1;
    // static-gradient outputs g0 of modality 0..3 = out0, out1, out2, aux2.
    // K_COST: scale = lr, lambda = beta1, inv_bg = beta2 (it also publishes this step's Adam lr_t).
    // K_LATENT / K_COST of a training step with a schedule set (avae_set_schedule): tail_w = the step's HyperEntry (below), which
    // replaces lambda and scales the KL weight (K_LATENT) / replaces scale = lr (K_COST).  Null otherwise, and in every evaluation
    // and inference launch: the by-value constants above are then all the item reads.
};

// One launch = up to kMaxItemsPerLaunch work items, passed BY VALUE in the kernel-argument
// segment together with the first block index of every item: a workgroup finds and reads its item
// without a chain of dependent loads from HBM, and no device-side table has to be kept in sync.
// Implicit-GEMM conv / transposed conv (reference vae_assoc.py:169-199,249-278, deconv.py:107): the patch matrix
//   P[(b,oh,ow)][(kh,kw,ci)] = X[b, (oh*so + kh - pad)/d, (ow*so + kw - pad)/d, ci]   (0 where not divisible / out of range)
// is never stored: a GEMM whose A operand is P computes the address of every 16-byte chunk it stages -- Cin*elem_size is a multiple
// of 16, so a chunk is 8 (bf16) / 4 (fp32) channels of ONE tap of one source pixel; an invalid tap reads a 16-byte block of
// zeros; the chunk at column K = k*k*Cin reads {1, 0, ...} when `ones` (the bias column of a stored patch matrix), zeros beyond.
// The LDS-DMA takes a per-lane source address, so the staged image is byte for byte the one a stored P would give.
// One geometry covers conv (so = stride, d = 1), transposed conv in gather form (so = 1, d = stride, pad = k-1-pad_before, the
// filter flipped in the matrix), flatten + dense (k = map size, VALID) and, with so <-> d swapped on the stage's OUTPUT gradient,
// every input gradient (adjoint form).  Divisions are multiplications by magic numbers (mg_x = floor(2^32 / x) + 1).
struct ConvA {
    const void* src;         // source map, compute dtype: element (b, pixel, c) at b*src_sb + pixel*src_sp + c
    const void* consts;      // [16 B of zeros][16 B {1, 0, ...} in the compute dtype]
    int M, K;                // rows B*OH*OW (rows beyond read zeros), k*k*Cin
    int OHW, OW, IH, IW, Cin;
    int k, so, d, pad;
    int src_sb, src_sp;
    int ones;
    unsigned mg_ohw, mg_ow, mg_k, mg_cin;
};
constexpr int kMaxConvA = 12;
constexpr int kMaxItemsPerLaunch = 12;
constexpr int kMaxPf = 4;
// Grid: x = tile slot inside an item (a multiple of 8, at least the largest item's tile count), y = item.
// A workgroup knows its item from blockIdx.y alone, so its WorkItem is ONE scalar-load round trip into the
// kernel-argument segment away; workgroups beyond their item's last tile exit at once.
struct LaunchArgs {
    int n_items;
    int grid_x;
    int sched;               // diagnostics (AVAE_SCHED): 0 = the shipped in-loop order of the 8-wave tiles, 1 = round 1's order
    int n_pf;                // 8-wave NT tiles: weight panels of the NEXT launch to pull into the Infinity Cache (0..kMaxPf)
    const void* pf_ptr[4];   // ... their first bytes
    int pf_lines[4];         // ... and sizes in 128-byte lines
    const ConvA* conv_tab;   // device table of the launch's implicit patch matrices (WorkItem::conv indexes it; null: none)
    WorkItem items[kMaxItemsPerLaunch];
};

// The weight-gradient launches (K-major operands, K_WGRAD only) carry a compact item: 80 bytes instead of 192, so every
// weight gradient of a step fits ONE launch's kernel-argument segment (4 KiB) and the tiles of all layers share the CUs'
// rounds (C4: 800 tiles in 4 rounds of one launch instead of 2 + 2 rounds of two).
struct TnItem {
    const void* A;           // X_aug   [K = batch rows][lda]
    const void* B;           // dA      [K][ldb]
    float* out;              // fp32 gradient [M][ld0]; split-K: slice s at out + s*M*ld0
    int M, N, K;
    int lda, ldb, ld0;
    int tiles_m, tiles_n;
    int ksplit, kchunk;
    int bias_row;            // see WorkItem::bias_row
    int tile_off, tile_cnt;  // this entry covers tiles [tile_off, tile_off + tile_cnt) of the item's tile list: the host cuts
    int conv;                // items with many tiles into several entries so that the grid (x = longest entry) is not mostly padding.
                             // conv > 0: A (the K-major operand X) is the implicit patch matrix conv - 1 of TnLaunchArgs::conv_tab
    // k_small_tn with the optimiser in its epilogue (TnLaunchArgs::adam): the layer's two compute-dtype shadows
    void* W; void* Wt;       // [M][ldw] (dgrad operand), [N][ldt] (forward operand)
    int ldw, ldt;
};
constexpr int kMaxTnItems = 32;
constexpr int kTnPieces = 8;
struct TnPiece { unsigned short item, tile_off, cum_end, pad; };      // tiles [tile_off, ...) of items[item]; cum_end = positions of the XCD up to and including this piece
struct DevState;
struct TnLaunchArgs {
    int n_items;
    int grid_x;
    int xcd_group;           // G = 1, 2, 4 or 8 items share the 8 XCDs: each item's tiles run on 8/G of them (see k_grouped)
    int sched;               // as LaunchArgs::sched
    // Small nets, one replica: the Adam step rides in this launch (k_small_tn<CT, true>) -- a tile's gradient block is applied to the
    // parameters as it leaves the accumulators, and k_adam's launch disappears.  theta / m / v of an element sit at its gradient's
    // address + a constant number of floats (the four fp32 arrays share the master layout).
    int adam;
    long long d_theta, d_m, d_v;
    float beta1, beta2, eps;
    const DevState* st;      // lr_t of this step (published by the K_COST item earlier in the step)
    const ConvA* conv_tab;
    // k_small_tn, XCD-owned pieces (xcd_pieces = 1): `items` holds WHOLE layers and XCD c runs the tiles of pieces[c][0..] in that
    // order -- workgroup x (XCD x % 8, position x / 8 on it) serves the piece whose [previous cum_end, cum_end) holds its position.
    // A layer's tiles then meet in ONE L2 (or two, where a layer is cut to balance the XCDs): its X / dA column panels come from
    // HBM once instead of once per XCD (C2: 11.8 of the launch's 33.3 MB of reads were such re-reads).
    int xcd_pieces;
    TnPiece pieces[8][kTnPieces];
    TnItem items[kMaxTnItems];
};
static_assert(sizeof(TnLaunchArgs) <= 4096, "kernel arguments are passed by value: 4 KiB");

// Per-workgroup launch descriptors (small-net training plan: the k_small and k_small_tn launches of a step).  What a workgroup's
// prologue works out from its item -- the tile split over the XCDs, t / tiles_n, the operand rows of its tile -- depends on the
// plan alone, so the host resolves it once per workgroup and launch into ONE 64-byte record of a device table: the kernel reads
// record blockIdx.x in one scalar burst and goes on to its per-lane offsets.  Record x runs on XCD x % 8 (workgroups are dealt
// round-robin), so XCD ownership of a tile is the order of the records; the grid is exactly the tile count.  The table's address
// comes in the preloaded leading kernel arguments, and the launch before warms the records (DescWarm).
struct alignas(64) SmallDesc {        // k_small_desc: hidden forward / hidden dgrad, 32x32 tile (m0, n0)
    const unsigned char* a;          // A + m0 * lda * ES
    const unsigned char* b;          // B + n0 * ldb * ES
    void* out;                       // out0 + m0 * ld0 + n0
    const void* aux;                 // dgrad: aux0 + m0 * ldx + n0 (the stored output act' is taken of)
    int lda, ldb, ld0, ldx;
    int nk;                          // K tiles
    int mrem, nrem, xrem;            // M - m0, N - n0, ldx - n0
};
struct alignas(64) TnDesc {           // k_small_tn_desc: 64x64 tile (m0, n0) of one layer's weight gradient, Adam in the epilogue
    const unsigned char* a;          // A + m0 * ES
    const unsigned char* b;          // B + n0 * ES
    float* out;                      // gradient + m0 * ld0 + n0 (theta / m / v at + TnDescArgs::d_*)
    void* w;                         // W + m0 * ldw + n0
    void* wt;                        // Wt + n0 * ldt + m0
    int lda, ldb, ld0, ldw, ldt;
    unsigned ext;                    // K tiles | min(M - m0, 64) << 16 | min(N - n0, 64) << 24  (one dword: a scalar load has no narrower form)
    static constexpr unsigned pack(int nk, int mrem, int nrem) { return (unsigned)nk | (unsigned)(mrem < 64 ? mrem : 64) << 16 | (unsigned)(nrem < 64 ? nrem : 64) << 24; }
};
static_assert(sizeof(SmallDesc) == 64 && sizeof(TnDesc) == 64, "a descriptor is one cache line");
// The step's other three launches (output + loss, the two fused head launches) resolve more per workgroup than one line holds: their
// records are two lines, read in one scalar burst like the others (several 64-byte scalar loads issued together cost what one
// does).  Narrow values share a dword; a scalar load has no narrower form.
struct alignas(128) LossRec {         // k_loss_rec: 32x32 tile (m0, n0) of an output layer + its loss, or one tile of the latent item
    const unsigned char* a;          // A + m0 * lda * ES
    const unsigned char* b;          // B + n0 * ldb * ES
    void* out;                       // out0 + m0 * ld0 + n0 (the gradient w.r.t. the logits)
    const float* x;                  // aux0 + m0 * ldx + n0 (the exact fp32 input the loss compares with)
    float* slot;                     // partial + slot_base + t (the tile's cost partial)
    int lda, ldb, ld0, ldx;
    int nk;                          // K tiles
    int mrem, nrem, xrem;            // M - m0, N - n0, ldx - n0
    float scale;
    int binary;
    int item, tile;                  // item >= 0: no GEMM tile -- tile `tile` of the by-value K_LATENT item `item` (the launch's trailing LaunchArgs)
    int pad_[10];
};
struct alignas(128) HeadRec {         // k_head_rec / k_latb_rec: 32x64 head tile of row block m0, tail slice ts (WorkItem::tail_*)
    const unsigned char* a;          // A + m0 * lda * ES
    const unsigned char* b;          // B (all 64 columns of the head)
    void* out0;                      // head: mulv + m0 * ld0;  latb: dH + m0 * ld0  (stored by slice 0)
    void* out1;                      // head: Z + m0 * ld1 (slice 0)
    const float* aux;                // head: eps + m0 * ldx;  latb: g0 + m0 * 3 * roundup(nz, 4)
    const unsigned char* tail_w;     // the consuming layer's weight shadow (whole: rows are clamped at tail_n - 1)
    void* tail_out;                  // tail_out + m0 * tail_ldo
    const void* tail_aux;            // latb: tail_aux + m0 * tail_ldx
    int lda, ldb, ld0, ld1, ldx;
    int tail_ldw, tail_ldo, tail_ldx;
    int nk, nz;
    int mrem;                        // M - m0
    int tail_n;
    unsigned tk;                     // tail_kt | slice index << 8 (slice 0 also stores the head's own results)
    int item;                        // item >= 0: no GEMM tile -- the by-value K_COST item `item` (the launch's trailing LaunchArgs)
    int pad_[2];
    static constexpr unsigned pack(int tail_kt, int ts) { return (unsigned)tail_kt | (unsigned)ts << 8; }
};
static_assert(sizeof(LossRec) == 128 && sizeof(HeadRec) == 128, "a head or loss record is two cache lines");
static_assert(sizeof(LaunchArgs) + 64 <= 4096, "the record kernels pass LaunchArgs by value behind their leading arguments: 4 KiB");
// The records the NEXT launch of the run will read, as n 64-byte lines from `lines` on: wave `wave` of workgroup x of this launch
// makes touch i = (x & 7) + 8 * (4 * (x >> 3) + wave).  One-line records: touch i is line i = record i.  Two-line records
// (kWarmPairs set in n): touch i is line 2 r + h of record r = (i & 7) + 8 * (i >> 4), h = (i >> 3) & 1.  Either way r % 8 = x % 8:
// a workgroup on this XCD will read the record, so the line waits in that XCD's L2.  A speed matter only: n = 0, or a line nobody
// warmed, is the cold read it always was.
constexpr int kWarmPairs = 1 << 30;
struct DescWarm { const void* lines; int n; };
struct TnDescArgs {                   // launch-wide constants of k_small_tn_desc (TnLaunchArgs' of the same names)
    long long d_theta, d_m, d_v;
    float beta1, beta2, eps;
    const DevState* st;
};
// They are the first kTnDescHead lines of that launch's table, one copy per XCD (workgroup x reads copy x & 7, which the launch
// before warmed on that XCD like any record); record x is line kTnDescHead + x, so it still runs on XCD (line index) % 8.
constexpr int kTnDescHead = 8;
static_assert(sizeof(TnDescArgs) <= 64, "a copy of the constants is one line of the table");

struct DevState {
    long long step;          // number of applied Adam steps
    float last_cost;
    float lr_t;              // lr*sqrt(1-b2^t)/(1-b1^t) of the step being applied (written by K_COST)
    float cost_hist[kCostHist];
};

// Global-norm clipping and non-finite step skipping (include/avae.h, avae_set_grad_clip): a first-use allocation of its own.
// max_norm / skip_nonfinite are read by the kernels, so changing their values re-captures no graph.
struct ClipState {
    float max_norm;                    // 0: no clipping; +inf: monitor only
    int skip_nonfinite;
    long long n_skipped;               // steps whose update was skipped
    float partial[kSumsqMaxBlocks];    // k_grad_sumsq's per-workgroup sums of this step (entries >= G stay zero)
    float norm_hist[kCostHist];        // raw gradient norm of every step, indexed like DevState::cost_hist
};

// Parameter averaging (include/avae.h, avae_set_ema): a first-use allocation of its own -- this header, then the average itself,
// P_int floats in the master layout (element i of theta has its average at avg[i]).  decay / warmup are read by k_adam, so changing
// their values re-captures no graph.
struct EmaState {
    float decay;
    int warmup;
    int pad[30];                       // the average starts on a 128-byte line, as theta does
};
static_assert(sizeof(EmaState) == 128, "the average is line-aligned behind its settings");

// Training schedules (include/avae.h, avae_set_schedule): a first-use allocation of its own.  The staging launch of a training
// submission evaluates the three schedules for each of its batches (step number = DevState::step + 1 + the batch's index) and
// writes entry j of `tab` -- read by the latent and cost items of the step on staging set j -- and the history ring.  The schedules
// themselves are read by that launch, so changing their values re-captures no graph.
struct HyperEntry { float kl, lambda, lr, pad; };      // kl_t, lambda_t = fl32(assoc_lambda * a_t), lr_eff_t = fl32(learning_rate * l_t)
constexpr int kHyperSets = 16;         // = the staging sets (kMultiSteps in avae_host.hip)
struct SchedState {
    avae_schedule sched[3];            // kl, assoc, lr
    float lambda0, lr0;                // cfg.assoc_lambda, cfg.learning_rate
    HyperEntry tab[kHyperSets];
    float hist[kCostHist][3];          // {kl_t, lambda_t, lr_eff_t} of every step, indexed like DevState::cost_hist
};

// Multiplier of schedule s at step number t (the number the update gets: 1 for the first step; u = t - 1 counts the steps before
// it) -- the ONE evaluator, used by avae_schedule_value on the host and by the staging kernel on the device.  The piecewise value is
// IEEE double arithmetic without contraction, rounded once: host and device agree in every bit.  EXP goes through pow(double).
// `s` has passed check_schedule (avae_host.hip).
__host__ __device__ inline float schedule_value(const avae_schedule& s, long long t) {
#pragma clang fp contract(off)
    long long u = t - 1;
    if (u < 0) u = 0;
    if (s.kind == AVAE_SCHED_PIECEWISE) {
        if (s.period > 0) u %= s.period;
        const int last = s.n_knots - 1;
        if (u <= s.knot_step[0]) return s.knot_value[0];
        if (u >= s.knot_step[last]) return s.knot_value[last];
        int i = 0;
        while (i + 1 < last && u >= s.knot_step[i + 1]) ++i;
        const double v0 = (double)s.knot_value[i], v1 = (double)s.knot_value[i + 1];
        const double f = (double)(u - s.knot_step[i]) / (double)(s.knot_step[i + 1] - s.knot_step[i]);
        return (float)(v0 + (v1 - v0) * f);
    }
    if (s.kind == AVAE_SCHED_EXP) {
        const double e = s.staircase ? (double)(u / s.decay_steps) : (double)u / (double)s.decay_steps;
        return (float)pow((double)s.decay_rate, e);
    }
    return 1.0f;
}

// One dense layer's optimiser tile table entry (Adam + compute-dtype shadow refresh).
struct AdamItem {
    float* theta;
    float* m;
    float* v;
    const float* g;
    void* W;                 // shadow [in+1 (padded)][ld]   : B operand of dgrad
    void* Wt;                // shadow [out (padded)][ldt]   : B operand of forward
    int rows, cols;          // in+1, out
    int ld, ldt;
    int tiles_r, tiles_c, tile_base;
    int ldw;                 // leading dim of the W shadow (>= ld: see spread_ld in avae_host.hip)
    // transposed-conv stages on the adjoint-frame route (adj_k > 0): the same pass also writes the adjoint filter shadows k_wadj
    // used to build in a launch of its own -- element (row (kh_m, kw_m, ci), col co) of the matrix goes, with kh = k-1-kh_m,
    // kw = k-1-kw_m and r = (kh*k + kw)*cols + co, to Wadj[ci][r] and Wf[r][ci]
    void* Wadj; void* Wf;
    int ldadj, ldf, adj_k, adj_cin;
};

constexpr int kMaxAdamItems = 80;      // kMaxMod * (2*AVAE_MAX_HIDDEN + 2)
struct AdamArgs {
    const AdamItem* items;
    int n_items;
    int base[kMaxAdamItems];           // first tile of every item (by value: no dependent scan through HBM)
    int mode;                // 0: Adam update; 1: refresh shadows from theta only
    int book;                // 1: this launch books the step's cost (last_cost, cost history)
    float lr, beta1, beta2, eps;
    DevState* st;
    const float* cost_src;   // grad[cost slot]
    ClipState* clip;         // k_adam<.., CLIP = true> only: the step's partial sums of squares, the threshold, the norm ring
    int n_partial;           // ... and how many partials there are (G)
    // k_adam<.., EMA = true> only (avae_set_ema): the average of the element at theta0 + i is avg[i].  mode 0: it is updated from
    // the new theta (decay / warmup from *ema); mode 1: the shadows are rebuilt from it instead of theta (avae_use_averaged)
    const EmaState* ema;
    float* avg;
    const float* theta0;
};

// Input staging ("prep"): fp32 rows -> compute-dtype copy (+ exact fp32 copy for the losses),
// and the eps tensor (copied from the caller or generated with Philox4x32-10).
struct PrepSeg {
    const float* src; int src_ld;
    int rows, cols;
    float* dst32; int ld32;        // nullable
    void* dstc; int ldc;           // row-major compute dtype
    int tiles_r, tiles_c, tile_base;
    // denoising staging (PrepArgs::noisy; include/avae.h, avae_set_corruption): dst32 keeps the rows of src (the loss target), dstc
    // gets the encoder's input -- the rows of src_in where the caller gave them, else src corrupted element by element: dropped
    // (-> drop_value) where the top 24 bits of the element's Philox word are below drop_thr, else + noise_std * N(0,1)
    const float* src_in; int in_ld;    // nullable
    unsigned drop_thr;                 // floor(drop_prob * 2^24); 0 = no drop stream
    float drop_value, noise_std;       // noise_std 0 = no noise stream
};
struct PrepArgs {
    PrepSeg seg[kMaxMod];
    int n_seg;
    int total_tiles;               // tiles of all segments; eps blocks follow
    // eps
    const float* eps_src;          // nullable -> Philox
    float* eps_dst;                // nullable -> no eps work
    int eps_rows, nz, eps_blocks, eps_ld;   // eps_ld = roundup(nz, 4): row stride of the internal eps buffer
    int row_offset;
    unsigned long long seed;
    const DevState* st;
    unsigned long long stream_salt;   // distinguishes train / eval / reconstruct draws
    // batched staging (avae_train_steps): the launch stages n_steps consecutive batches at once.  Batch j reads rows
    // [j*rows, (j+1)*rows) of every source (and of eps_src), writes staging set j (every destination moved by
    // j*set_stride bytes) and draws eps for step st->step + j.  blocks_per_step = total_tiles + eps_blocks.
    int n_steps, blocks_per_step;
    long long set_stride;
    // masked staging (nullable; null = the unmasked staging above, unchanged): caller's presence bytes [n_steps*rows][pres_ld],
    // nonzero = observed.  An absent (row, modality) -- and every row of a null seg[m].src -- is staged as zeros; the blocks of
    // segment 0's first column tile copy the presence (0/1, a null source folded in) into set j of pres_dst at j*rows*pres_ld.
    const unsigned char* pres_src;
    unsigned char* pres_dst;
    int pres_ld;
    int noisy;                     // some segment has a second source or a corruption: the NOISY instances (else the two above, unchanged)
    SchedState* sched;             // training staging with a schedule set (the SCHED instances; null: the instances above, unchanged):
                                   // thread 0 of batch j's first block writes tab[j] and the history entry of step st->step + 1 + j
};

// Fixed-order sum of the split-K slices of a weight gradient: dst[i] = sum_s src[s*stride + i]  (no atomics: reproducible).
struct ReduceSeg { float* dst; const float* src; int n, parts; long long stride; int block_base;
                   int dst_ld;      // dst_ld > 0: element i goes to dst[i * dst_ld] (a one-column gradient in a padded matrix)
                   int colsum;      // 1: k_colsum's tree (many short partial vectors), 0: k_reduce's slice sum -- one launch may carry both (k_sums)
                   // slice sums of an adjoint-frame filter gradient [Cin][(kh', kw', co)] (leading dim perm_ldga) go straight to the
                   // gradient buffer's layout [(kh, kw, ci)][co] (leading dim perm_ld, kh = k-1-kh'): perm_k > 0, dst = that matrix
                   int perm_k, perm_cin, perm_cout, perm_ldga, perm_ld; };
constexpr int kMaxReduceSegs = 40;          // up to 9 split conv stages per modality x 4 modalities (+ bias sums)
struct ReduceArgs { ReduceSeg seg[kMaxReduceSegs]; int n_seg; };

// Conv / transposed-conv layers (reference vae_assoc.py:169-199,249-278, deconv.py:107) run on the
// same GEMM kernel through explicit patch matrices.  One geometry covers both directions:
//   P[(b,oh,ow)][(kh,kw,ci)] = X[b, (oh*so + kh - pad)/d, (ow*so + kw - pad)/d, ci]   (0 if not divisible / out of range)
// conv: so = stride, d = 1, pad = TF pad-before;  transposed conv: so = 1, d = stride, pad = k-1-pad_before with
// the filter flipped when it is laid out as a matrix;  flatten+dense: k = map size, VALID.
struct ConvGeom {
    int B, IH, IW, Cin, OH, OW, k, so, d, pad;
    int src_sb, src_sp;        // element strides of the source: batch, pixel (channel stride 1)
    int ones;                  // append the constant-1 bias column at index k*k*Cin
};
// k_gather (im2col): source activations -> patch matrix P (row-major + transposed), compute dtype
struct GatherSeg {
    ConvGeom g;
    const void* src;
    void* P; int ldp;
    int tiles_r, tiles_c, tile_base;
    int cl, rpt;                      // tile shape, see Col2imSeg
};
struct GatherArgs { GatherSeg seg[kMaxMod]; int n_seg; };
// k_col2im: fp32 patch gradients dP -> gradient of the layer input, times act'(stored input), written
// row-major + transposed in the compute dtype; latent mode turns dz into [dmu | dlv] (reparameterisation).
struct Col2imSeg {
    ConvGeom g;
    const float* dP; int lddp;
    const void* yprev; int ldy;      // stored output of the producing layer (nullable -> identity)
    int act;                          // AVAE_ACT_* of the producing layer
    void* dA; int lda;                // [B*IH*IW][lda]
    const float* g0; int nz;          // latent mode when g0 != nullptr
    const void* bias; int bias_ld;    // forward mode when bias != nullptr (a transposed conv as scatter product + overlap-add):
                                      // dA = act(sum + bias[c * bias_ld]) instead of sum * act'(yprev)
    int tiles_r, tiles_c, tile_base;
    int cl, rpt;                      // tile shape: cl (1..16, power of two) lanes of 4 columns, rpt (1 or 4) rows per thread:
                                      // (256/cl)*rpt rows x 4*cl columns -- narrow outputs get tall tiles, short ones many tiles
};
struct Col2imArgs { Col2imSeg seg[kMaxMod]; int n_seg; };

// The last transposed-conv stage (G2 channels -> ONE 28x28 map, vae_assoc.py:274-278) as direct kernels.  On the GEMM path
// its single output channel is one useful column of a 32-wide tile, its patch matrix is 180 MB and its fp32 patch gradients
// 321 MB per step at batch 256; computed directly the stage reads its 1.6 MB input and the 400 filter taps.
// One workgroup per image, the image staged in LDS:
//   mode 0  forward    : Y[p] = act(bias + sum_taps X[b, ih, iw, :] . F[kh, kw, :])
//   mode 1  input grad : dX[b, ih, iw, c] = act_in'(X) * sum_taps dY[b, oh, ow] * F[kh, kw, c]
//   mode 2  filter grad: part[image][Kp]   (summed over images by k_colsum)
constexpr int kThinIn = 4096, kThinOut = 1024, kThinF = 1024;   // k_thin: one image staged in LDS (floats)
constexpr int kThinSplit = 4;          // workgroups per image (each stages the image and takes a quarter of the outputs): one
                                       // workgroup per CU leaves the LDS latency of these loops exposed
struct ThinSeg {
    ConvGeom g;
    const void* X;           // stage input = stored output of the producing stage, [b*src_sb + pixel*src_sp + c]
    const void* Wt;          // filter shadow [1][ldt]: taps (kh, kw, c), bias at index k*k*Cin
    void* Y; int ldy;        // stage output, column 0 of [rows][ldy]
    int act, act_in;         // transfer function of this stage / of the producing stage
    const void* dY; int lddy;   // gradient w.r.t. this stage's pre-activation output, column 0
    void* dX; int lddx;      // gradient w.r.t. the producing stage's pre-activation output [pixels][lddx]
    float* part;             // mode 2: [blocks][Kp]
    int Kp;                  // roundup(k*k*Cin + 1, 4)
    int block_base;
    int img_y, img_dy;       // > 0: elements from one image's map to the next in Y / dY (dense rows); 0: OH*OW*ldy / OH*OW*lddy
    int split;               // workgroups per image: kThinSplit, or 1 on the block-structured path below
    int fast;                // the reference's geometry (k 5, stride-2 transposed conv in gather form: so 1, d 2, pad 3, OH = 2 IH, 8 or 16
                             // input channels): one workgroup per image; forward = a thread per 2x2 output block over its 3x3 input
                             // neighbourhood (every tap test folds at compile time), input gradient = a thread per (pixel, channel quad)
                             // over the 5x5 window, filter gradient = a thread per (tap, tenth of the pixels) for all channels
};
inline bool thin_fast_geometry(const ConvGeom& g) {
    return g.k == 5 && g.so == 1 && g.d == 2 && g.pad == 3 && g.OH == 2 * g.IH && g.OW == 2 * g.IW && (g.Cin == 8 || g.Cin == 16) && g.ones;
}
struct ThinArgs { ThinSeg seg[kMaxMod]; int n_seg; int mode; };
void launch_thin(int compute_dtype, const ThinArgs& a, int n_blocks, hipStream_t s);
void launch_colsum(const ReduceArgs& a, int n_blocks, hipStream_t s);

// Adjoint filter shadow of a transposed-conv stage: Wadj[ci][(kh', kw', co)] = Wt[co][((k-1-kh')*k + (k-1-kw'))*Cin + ci], the B
// operand of the stage's input gradient computed as a GEMM on the patch matrix of its OUTPUT gradient.
// ... and its transpose Wf[(kh', kw', co)][ci], the B operand of the stage's FORWARD pass as a scatter product (below).
struct WadjSeg { const void* Wt; void* Wadj; void* Wf; int ldt, ldadj, ldf, k, Cin, Cout, block_base; };
struct WadjArgs { WadjSeg seg[2 * kMaxMod]; int n_seg; };
void launch_wadj(int compute_dtype, const WadjArgs& a, int n_blocks, hipStream_t s);
// Filter gradient of such a stage, computed in the adjoint frame Gadj[ci][(kh', kw', co)] = sum_pixels X[p][ci] * Padj[p][...],
// moved into the gradient buffer's layout G[(kh, kw, ci)][co] (kh = k-1-kh').
struct GpermSeg { const float* Gadj; float* G; int ldga, ld, k, Cin, Cout, block_base; };
struct GpermArgs { GpermSeg seg[2 * kMaxMod]; int n_seg; };
void launch_gperm(const GpermArgs& a, int n_blocks, hipStream_t s);
// Column sums of a compute-type matrix, first level: workgroup j adds rows j, j + blocks, ... -> part[j][cols4] (the bias
// gradient of a conv stage = column sums of its output gradient; k_colsum adds the partial sums in order).
struct RowsumSeg { const void* src; float* part; int ld, rows, cols, cols4, cpow, n_blocks, block_base; };
struct RowsumArgs { RowsumSeg seg[2 * kMaxMod]; int n_seg; };
void launch_rowsum(int compute_dtype, const RowsumArgs& a, int n_blocks, hipStream_t s);

// Serving (avae_generate): the captured decode graph's output launch reads the caller's pointers and row count from this
// device-side slot (written by the per-call staging launch), so that one graph serves every call without re-parameterising its nodes.
struct ServeSlot {
    const float* z;                // [rows][n_z] fp32, dense
    float* out[kMaxMod];           // per modality [rows][n_input] fp32, dense
    int rows;
    int pad;
};
struct ServeArgs {               // the per-call staging launch: z -> Z of every modality (rows beyond the call's rows zero)
    ServeSlot* slot;
    int n_mod, nz, bucket;         // rows of the captured plan (>= the call's rows)
    void* Z[kMaxMod]; int ldz[kMaxMod];            // decoder inputs, compute dtype, [bucket][ldz]
    int blocks_per_mod;
};
void launch_serve(int compute_dtype, const ServeArgs& a, const ServeSlot& call, int n_blocks, hipStream_t s);
// k_serve_in: the staging launch that also runs the decoder's first layer (small nets)
struct ServeInMod { const void* w; void* out; int n, ldw, ldo, kt, act, slices; };   // first decoder layer of one modality: weight shadow [n][ldw], output [bucket][ldo]
struct ServeInArgs {
    ServeSlot call;                // this call's pointers and row count (by value: one launch per call)
    ServeSlot* slot;               // where the plan's output launch reads them
    int n_mod, nz, bucket, tiles_m;
    ServeInMod mod[kMaxMod];
};
void launch_serve_in(int compute_dtype, const ServeInArgs& a, int grid_x, hipStream_t s);

void launch_gather(int compute_dtype, const GatherArgs& a, int n_blocks, hipStream_t s);
void launch_col2im(int compute_dtype, const Col2imArgs& a, int n_blocks, hipStream_t s);

// Per-row scoring (avae_score): one wave64 per row, kScoreRows rows per workgroup; every sum is a fixed-order shuffle tree (no
// atomics), so a row's score does not depend on the chunking or the launch shape.  Score rows are dense [rows][k] fp32 in the
// order cost | recon[M] | latent[M] | assoc[P] | cross[s*M+d].
constexpr int kScoreRows = kThreads / 64;
struct ScoreLatentArgs {
    const float* mulv[kMaxMod];    // [rows][2*n_z] fp32: [mu | log sigma^2] of every modality
    void* Z[kMaxMod]; int ldz[kMaxMod];            // decoder inputs, compute dtype, [rows][ldz] (columns [0, n_z) written)
    const float* eps; int ld_eps;  // [rows][ld_eps] fp32 (the sampled pass)
    float* out; int k;             // score rows
    int rows, nz, n_mod;
    int src;                       // < 0: sampled pass (latent, assoc columns; z_m = mu_m + exp(lv_m/2) eps); else z = mu_src for every decoder
    // masked scoring (avae_score_masked; nullable, null = the unmasked kernel): the chunk's staged presence bytes [rows][n_mod],
    // 0 / 1.  An absent modality's latent column and every pair column it is part of hold +0.0, its decoder input zeros.
    const unsigned char* present;
};
void launch_score_latent(int compute_dtype, const ScoreLatentArgs& a, hipStream_t s);
struct ScoreRowsArgs {
    const float* xhat; int ld32;   // decoder output of this pass: p (Bernoulli) or x_hat (Gaussian), fp32 [rows][ld32]
    const float* x; long long ldx; // the caller's rows of that modality
    float* out; int k;
    int rows, n_in, binary, col;   // score column of this pass
    int cost;                      // 1: also cost = sum_m w_m (recon_m + latent_m) + lambda sum_p assoc_p (the sampled pass's last modality)
    int n_mod, n_pair;
    float w[kMaxMod]; float lambda;
    // masked scoring (nullable): presence bytes as above.  The column holds the unmasked value where the row has modalities pa and
    // pb (pa == pb for a recon column), else absent_bits (+0.0 for recon, quiet NaN for cross); an absent row's x is never loaded.
    const unsigned char* present; int pa, pb; unsigned absent_bits;
};
void launch_score_rows(const ScoreRowsArgs& a, hipStream_t s);

// Importance-weighted log-likelihoods (avae_loglik).  A pass decodes rows * kc latent samples of ONE proposal src: decoded row
// i = j * kc + k holds input row j (of the pass) and sample k0 + k.  Same shapes and no-atomics rule as the score kernels.
struct IwLatentArgs {
    const float* mulv;              // [rows][2*n_z] fp32 of the proposal's modality
    const float* eps;               // caller's [all rows][K][n_z] fp32, at the pass's first input row; NULL: Philox
    float* z32;                     // NULL, or [n_dec][n_z] fp32 (the serve route reads it)
    void* Z[kMaxMod]; int ldz[kMaxMod]; int n_zdst;   // decoder inputs, compute dtype (the modality-by-modality route)
    float* r;                       // [n_dec] log N(z;0,I) - log q(z|x)
    int rows, kc, k0, K, nz;
    long long row0;                 // Philox: row of the whole input of the pass's first row (row_offset included)
    unsigned long long seed; unsigned draw;
    // masked log-likelihood (avae_loglik_masked; nullable): the proposal's column of the chunk's staged presence bytes, row stride
    // pres_ld.  A row without the proposal's modality draws nothing: its decoder inputs are zeros and its r is NaN.
    const unsigned char* present; int pres_ld;
};
void launch_iw_latent(int compute_dtype, const IwLatentArgs& a, hipStream_t s);
struct IwRowsArgs {
    const float* xhat[kMaxMod]; int ldh[kMaxMod];           // decoder outputs (p or x_hat) fp32, [n_dec][ldh]
    const float* x[kMaxMod]; long long ldx[kMaxMod];        // the caller's rows, at the pass's first input row
    int n_in[kMaxMod], binary[kMaxMod];
    float* ell;                     // [n_dec][n_mod]: -recon
    int n_dec, kc, n_mod;
    const unsigned char* present;   // masked (nullable): [rows][n_mod]; an absent target's x is never loaded, its ell holds +0.0
};
void launch_iw_rows(const IwRowsArgs& a, hipStream_t s);
struct IwReduceArgs {
    const float* ell; const float* r;   // this pass's [n_dec][n_mod], [n_dec]
    float* state;                   // [rows][n_mod][2 + n_mod][2] running (max, sum exp) per input row of the chunk
    float* out; int width;          // the caller's rows [rows][width] at the pass's first input row
    int rows, kc, src, n_mod;
    int first, last;                // first / last sample block of the row
    float log_k;
    // masked (nullable): [rows][n_mod].  A row without the proposal writes NaN to all its outputs of this proposal and keeps no
    // state; else an absent target d stays out of the joint sum, its conditional is NaN and its running state is not touched.
    const unsigned char* present;
};
void launch_iw_reduce(const IwReduceArgs& a, hipStream_t s);

// Fused-posterior prediction (avae_impute).  k_impute_fuse: one wave64 per row, one lane per latent dimension; the Gaussian closest
// to the present modalities' posteriors in sum_m KL(q || q_m): precision = mean of the precisions, mean precision-weighted,
// max-shifted so exp stays in range.  One present modality is a select of its (mu, lv), none is the prior (+0.0, +0.0).
struct ImputeFuseArgs {
    const float* mulv[kMaxMod];    // [rows][2*n_z] fp32 of every modality (a modality outside `mods` is never read)
    unsigned mods;                 // bit m: x_dev[m] was given (the presence of every row when `present` is NULL)
    const unsigned char* present;  // NULL, or the chunk's staged presence bytes [rows][n_mod], 0 / 1, NULL sources folded in
    float* fused;                  // [rows][2*n_z] fp32 [mu_f | lv_f]: the proposal k_iw_latent samples from
    float* mu; float* lv;          // nullable: the caller's [rows][n_z] rows of this chunk
    float* z32;                    // n_samples = 0 (nullable): mu_f as dense fp32 z rows (the serve route) ...
    void* Z[kMaxMod]; int ldz[kMaxMod]; int n_zdst;   // ... or into every decoder input, compute dtype (the modality-by-modality route)
    int rows, nz, n_mod;
};
void launch_impute_fuse(int compute_dtype, const ImputeFuseArgs& a, hipStream_t s);
// k_impute_accum: one wave64 per (input row of the pass, modality, tile of 64 output columns), lanes on consecutive columns.
// Welford's update over the pass's kc decoded rows of that input row, sequentially in sample order, in registers; the running
// (mean, M2) crosses passes in `state`; the row's last sample block stores mean and M2 / K.  No atomics.
struct ImputeAccumArgs {
    const float* xhat[kMaxMod]; int ldh[kMaxMod];   // decoder outputs fp32, [n_dec][ldh], decoded row i = j * kc + k
    float* mean[kMaxMod]; float* var[kMaxMod];      // nullable: the caller's dense [rows][n_input] rows, at the pass's first input row
    int n_in[kMaxMod];
    int tile0[kMaxMod + 1];        // prefix sums of the modalities' column tiles
    int col0[kMaxMod];             // prefix sums of n_input: a modality's first column in a state row
    float* state; int ld_state;    // [rows][ld_state = sum n_input][2] running (mean, M2)
    int rows, kc, k0, K, n_mod;
};
void launch_impute_accum(const ImputeAccumArgs& a, hipStream_t s);

// ---- gradient exchange (avae_comm.hip)
// One-shot all-reduce over hipIpc peers ("a hand-rolled P2P reduce-scatter/all-gather over hipIpc peers"):
// every rank owns an exchange block (uncached device memory, mapped by every peer); a range of the gradient buffer is cut into
// `world` shards of 8-float granules, shard j is reduced by rank j:
//   phase 1  push     rank r stores its values of shard j into slot r of rank j's block           (all 7 links at once)
//   phase 2  reduce   rank j adds slots 0..world-1 in RANK ORDER (its own from g), stores the sum into every rank's result area
//   phase 3  collect  every rank copies the other shards' sums from its result area into g
// Workgroup w of every rank works on chunk w of every shard and signals / waits on workgroup w of its peers only (a flag word per
// (workgroup, source rank), value = the call's sequence number), so there is no grid barrier and no reset; every wait is bounded by
// a wall-clock timeout that raises the block's error word instead of hanging.  Cross-GPU traffic is stores only (posted writes).
constexpr int kMaxWorld = 8;
constexpr int kIpcThreads = 256;
struct IpcArgs {
    float* g;                       // local gradient buffer (master layout + cost slot)
    long long off, granules;        // range = floats [off, off + 8*granules)
    long long cost_idx;             // >= 0: g[cost_idx] is summed over the ranks in fp32 beside the range
    int world, rank, wire_bf16, blocks;
    unsigned char* peer[kMaxWorld]; // every rank's exchange block as mapped in this process (peer[rank] = the own block)
    long long off_flag1, off_flag2; // unsigned [blocks][kMaxWorld]: flag of (workgroup, source rank)
    long long off_cost;             // float [kMaxWorld]: the ranks' local costs
    long long off_seq;              // unsigned [blocks]: calls completed by workgroup w (local use only)
    long long off_err;              // unsigned: nonzero after a timed-out wait (local use only)
    long long off_slots, slot_stride, off_res;   // bytes
    unsigned long long timeout_ticks;            // of the 100 MHz wall clock
};
void launch_ipc_allreduce(const IpcArgs& a, hipStream_t s);
// bf16 wire format for the RCCL path: gradient range -> bf16 wire buffer, and back after the all-reduce
void launch_wire_pack(const float* g, void* wire, long long n, hipStream_t s);
void launch_wire_unpack(float* g, const void* wire, long long n, hipStream_t s);

// Diagnostic build only (-DAVAE_STAMPS): thread 0 of every block records s_memrealtime (100 MHz)
// at kernel entry / after the item lookup / after the first staged tile / after the K loop / at
// the end, plus s_memtime (shader clock) at entry and end.  No stamp executes in the product build.
struct LaunchEvents { hipEvent_t start, stop; };
extern thread_local LaunchEvents t_launch_events;   // armed by the host in timing mode, consumed by the next launch
// Every kernel launch of the library: the one place that knows the two modes (timing mode: avae_kernels.hip, at t_launch_events).
template <typename K, typename... Args>
void launch_kernel(K kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const Args&... args) {
    if (t_launch_events.start) {
        hipExtLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, t_launch_events.start, t_launch_events.stop, 0, args...);
        t_launch_events = LaunchEvents{nullptr, nullptr};
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
    }
}
// The LDS of one CU, all of which a kernel may ask for as dynamic LDS -- once it has opted in: more than 64 KiB has to be allowed
// per kernel (cheap to repeat).
constexpr size_t kMaxDynLds = 160 * 1024;
template <typename K> void allow_max_lds(K kernel) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxDynLds);
}

constexpr int kStampLaunches = 32, kStampBlocks = 1024, kStampWords = 8;

// launchers implemented in avae_kernels.hip
int tile_lds_bytes(int tile_cfg, bool two_c_tiles);
void launch_grouped(int compute_dtype, int tile_cfg, const LaunchArgs& args, int grid_x, int grid_y, int lds_bytes,
                    DevState* st, hipStream_t s, unsigned long long* stamps = nullptr, int launch_id = 0);
void launch_grouped_tn(int compute_dtype, int tile_cfg, const TnLaunchArgs& args, int grid_x, int grid_y, int lds_bytes,
                       DevState* st, hipStream_t s, unsigned long long* stamps = nullptr, int launch_id = 0);
void launch_adam(int compute_dtype, const AdamArgs& a, int n_blocks, hipStream_t s);      // a.clip != null: the clip-aware instance; a.avg != null: the averaging one
void launch_grad_sumsq(const float* g, long long p_int, float* partial, hipStream_t s);
void launch_prep(int compute_dtype, const PrepArgs& a, hipStream_t s);
const void* prep_kernel(int compute_dtype, bool masked, bool noisy, bool sched);   // for hipGraphExecKernelNodeSetParams on the captured staging node
void launch_fill(void* base, int elem_bytes, unsigned bits, long long start, long long stride, int count, hipStream_t s);
void launch_sums(const ReduceArgs& a, int n_blocks, hipStream_t s);
int small_head_lds_bytes();
void launch_small_latb(int compute_dtype, int act, const LaunchArgs& args, int grid_x, int grid_y, int lds_bytes, DevState* st, hipStream_t s,
                       unsigned long long* stamps, int launch_id);
void launch_small_head(int compute_dtype, int act, const LaunchArgs& args, int grid_x, int grid_y, int lds_bytes, hipStream_t s,
                       unsigned long long* stamps, int launch_id);
void launch_small_tn(int compute_dtype, const TnLaunchArgs& args, int grid_x, int grid_y, hipStream_t s, unsigned long long* stamps, int launch_id);
void launch_small_loss(int compute_dtype, const LaunchArgs& args, int grid_x, int grid_y, int lds_bytes, hipStream_t s, unsigned long long* stamps, int launch_id);
void launch_small(int compute_dtype, const LaunchArgs& args, int grid_x, int grid_y, int lds_bytes, hipStream_t s, unsigned long long* stamps, int launch_id);
void launch_small_desc(int compute_dtype, bool dgrad, int act, const SmallDesc* tab, int n_tiles, int lds_bytes, DescWarm warm, hipStream_t s,
                       unsigned long long* stamps, int launch_id);
void launch_small_tn_desc(int compute_dtype, const TnDesc* tab, int n_tiles, bool grad, DescWarm warm, hipStream_t s, unsigned long long* stamps, int launch_id);
// the output + loss and the two head launches of the training plan on records; `args` rides along for the latent / cost item alone
void launch_loss_rec(int compute_dtype, const LossRec* tab, int n_recs, int lds_bytes, DescWarm warm, const LaunchArgs& args, hipStream_t s,
                     unsigned long long* stamps, int launch_id);
void launch_head_rec(int compute_dtype, int act, const HeadRec* tab, int n_recs, int lds_bytes, DescWarm warm, hipStream_t s,
                     unsigned long long* stamps, int launch_id);
void launch_latb_rec(int compute_dtype, int act, const HeadRec* tab, int n_recs, int lds_bytes, DescWarm warm, DevState* st, const LaunchArgs& args,
                     hipStream_t s, unsigned long long* stamps, int launch_id);
void launch_reduce(const ReduceArgs& a, int n_blocks, hipStream_t s);
void launch_chain2(int compute_dtype, const LaunchArgs& args, int grid_x, int grid_y, int lds_bytes, unsigned* counters, unsigned* err, hipStream_t s);

}  // namespace avae
