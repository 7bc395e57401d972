// Host side of libavae: memory plan, work-item tables, hipGraph capture and the C ABI
// (include/avae.h).  No per-step allocation: everything is carved once from one workspace.
#include "avae_device.h"
#include "avae_complete.h"
#include "avae_retrieve.h"
#include "avae_latent_stats.h"
#include "avae_motion.h"
#include "avae_render.h"
#include "avae_grad.h"
#include "avae_thumbnail.h"
#include "avae_ik.h"
#include "avae_dynamics.h"
#include "avae_lognormal.h"
#include "avae_track.h"
#include "avae_search.h"
#include "avae_gmm.h"
#include "avae_embed.h"
#include "avae_aggpost.h"
#include "../../include/avae.h"

#include <dlfcn.h>
#include <sched.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <cstddef>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

using namespace avae;

namespace {

thread_local std::string g_create_error;

struct Err : std::runtime_error { using std::runtime_error::runtime_error; };

#define HIP_OK(expr)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            throw Err(std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" +    \
                      std::to_string(__LINE__) + ")");                                           \
    } while (0)

// The calling thread's current HIP device is put back on exit: a process may hold a model on device k while its own (torch)
// current device is j, and every ABI call switching the thread to k would silently move the caller's later allocations.
struct DeviceGuard {
    int prev = -1, want = -1;
    explicit DeviceGuard(int dev) : want(dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != want) HIP_OK(hipSetDevice(want));
    }
    ~DeviceGuard() { if (prev >= 0 && prev != want) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// A launch rejected by the runtime (grid / LDS size, bad kernel arguments) must surface as this call's error, not later as a
// wrong number.  Also legal while a stream is being captured.
#define LAUNCH_OK(what)                                                                          \
    do {                                                                                         \
        hipError_t e_ = hipGetLastError();                                                       \
        if (e_ != hipSuccess) throw Err(std::string("launch of ") + (what) + ": " + hipGetErrorString(e_)); \
    } while (0)

constexpr unsigned long long kTrainSalt = 0x7261696eull;      // "rain": the eps stream of the training calls (PrepArgs::stream_salt)
static_assert(kHyperSets == 16, "one schedule table entry per staging set");
constexpr int kMultiSteps = 16;         // most whole steps per replay of a multi-step graph (avae_train_steps) = staging sets
constexpr int kMultiSizes[2] = {16, 4};  // captured replay lengths: a run of n batches goes 16,16,...,4,4,...,1,1

inline size_t rup(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ----------------------------------------------------------------------------- memory plan
struct Bump {
    size_t off = 0;
    size_t take(size_t bytes) { size_t o = off; off = rup(off + bytes, 256); return o; }
};

struct Dense {             // one dense layer, weights + bias as W_aug [(in+1)][ld]
    int in = 0, out = 0;
    int ld = 0;            // master (theta, m, v, g) leading dim = rup(out, KU)
    int ldw = 0;           // W-shadow leading dim: ld, or ld + KU where ld would be a channel-aliasing stride (spread_ld)
    int ldt = 0;           // W^T-shadow leading dim = rup(in+1, KU)
    size_t master = 0;     // offset in floats inside the theta/m/v/g regions
    size_t W = 0, Wt = 0;  // byte offsets in the workspace
    bool head = false;     // [mu|sigma] fused head: flat layout is Wmu,bmu,Wsig,bsig
};

constexpr int kRowsumBlocks = 256;   // workgroups of the bias-gradient row sums (k_rowsum)

struct Act {               // activation or gradient: row-major [rows p][ld] (every consumer reads it as stored)
    int width = 0;
    int rows = 0;          // logical rows (batch, or batch * output pixels for a conv stage)
    int ld = 0;
    size_t rm = 0;
    bool ones = false;
};

// One conv-like stage of the conv/deconv branch: gather (im2col) -> GEMM on the patch matrix.
struct ConvStage {
    ConvGeom g{};          // for the training batch
    Dense d;               // in = k*k*Cin, out = Cout (W_aug: bias row only fed when `bias`)
    bool bias = false;
    int act = AVAE_ACT_IDENTITY;   // transfer function applied to this stage's output
    int flat = 0;          // flat-parameter form: 0 conv filter [k,k,ci,co] (no bias); 1 transposed-conv filter
                           // [k,k,co,ci] + bias[co]; 2 dense W[in,out] + b; 3 fused head Wmu,bmu,Wsig,bsig
    Act P;                 // patch matrix, rows = B*OH*OW, width = k*k*Cin
    Act Y;                 // stage output (row-major only), NHWC rows
    Act dY;                // gradient w.r.t. the stage's pre-activation output (row-major + transposed)
    size_t dP = 0;         // fp32 patch gradients [rows][lddp]
    int lddp = 0;
    int ksplit = 1, kchunk = 0;    // weight gradient: K = rows is cut into ksplit chunks of kchunk K tiles (see WorkItem)
    size_t part = 0;       // fp32 slices [ksplit][K+1][d.ld] of the split weight gradient
    bool adj = false;      // transposed conv whose input gradient is a GEMM on the patch matrix of its OUTPUT gradient
    Act Padj;              // that patch matrix, rows = B*IH*IW, width = k*k*Cout
    size_t Wadj = 0;       // adjoint filter shadow [Cin (padded)][ldadj]
    int ldadj = 0;
    size_t Wf = 0;         // its transpose [k*k*Cout (padded)][ldf]: B operand of the forward scatter product
    int ldf = 0;
    size_t T = 0;          // fp32 scatter product [B*IH*IW][ldT] = X . Wadj, overlap-added into Y by k_col2im (forward mode)
    int ldT = 0;
    size_t Gadj = 0;       // fp32 filter gradient in the adjoint frame [Cin][ldga] (+ aksplit slices at apart)
    int ldga = 0, aksplit = 1, akchunk = 0;
    size_t apart = 0;
    size_t rs_part = 0;    // bias gradient: partial column sums of dY [kRowsumBlocks][rs_cols4]
    int rs_cols4 = 0;
    // Implicit-GEMM routes of the training plan (ConvA, avae_device.h): the stage's patch matrix is never stored.
    bool impl = false;     // forward + filter gradient: A = implicit P of the stage's input (needs Cin * elem_size % 16 == 0)
    bool impl_w = false;   // filter gradient: dW = P^T . dY with P implicit (gather form on the stage's input); impl implies it (no stored P then)
    bool impl_bwd = false; // input gradient: A = implicit patch matrix of the stage's OUTPUT gradient with the adjoint geometry, B = Wadj
                           // (needs Cout * elem_size % 16 == 0 and an input that has a gradient)
    int cin_real = 0;      // channels of the stage's input in the flat parameter layout (the first decoder stage pads n_z up to a whole chunk)
    bool dense_map = false;// the direct one-channel 28x28 stage: its output / output gradient are stored as dense rows [B][784 (+1)],
                           // which makes the dense output layer behind it an ordinary dense layer (no flatten gather, no col2im)
    bool thin = false;     // one output channel: direct kernels (k_thin) instead of im2col -> GEMM -> col2im in the training plan
    size_t thin_part = 0;  // its filter-gradient partial sums [thin_blocks][Kp]
    int thin_blocks = 0, thin_kp = 0;
};

struct Mod {
    int n_in = 0, L = 0;
    std::vector<int> hs;
    std::vector<Dense> enc, dec;   // hidden layers
    Dense head, outl;
    Act X0, Z, dH, dO;
    std::vector<Act> E, D, dE, dD;
    size_t X32 = 0, mulv = 0, g0 = 0, out32 = 0;
    int ld32 = 0;
    bool conv = false;             // hidden_conv branch: cenc = E1,E2,E3,HEAD  cdec = T1,T2,T3,T4,OUT
    std::vector<ConvStage> cenc, cdec;
};

struct Launch {
    std::string name;
    LaunchType type = kGrouped;
    TileCfg cfg = k64x64;  // kGrouped launches only
    int first = 0, count = 0, blocks = 0, lds = 0;
    int lean_act = 0;      // kLeanLatb / kLeanHead: the tail's transfer function
    int grid_x = 1, grid_y = 1;   // grouped kernel: tile slot x item
    bool tn = false;              // K-major operands (the weight-gradient launches)
    LaunchArgs args{};
    TnLaunchArgs targs{};         // tn launches carry compact items instead
    // Per-workgroup descriptors (build_descriptors: the training plan's k_small and k_small_tn launches).  desc_n > 0: the launch runs
    // on desc_n records instead of its by-value arguments; staging set j's copy of them starts at byte desc_off + j * desc_stride of
    // the handle's table, and desc_set is the set this copy of the launch runs on (relocated()).
    int desc_n = 0, desc_set = 0;
    size_t desc_off = 0, desc_stride = 0;
    GatherArgs ga{};
    Col2imArgs ca{};
    ReduceArgs ra{};
    ThinArgs ta{};
    WadjArgs wa{};
    GpermArgs gp{};
    RowsumArgs rs{};
};

struct TimingRec { hipEvent_t a, b; int launch_name; };

// A captured graph; for a step graph also its template and its staging-kernel root node, kept so that the caller's pointers can be
// patched in before a replay (hipGraphExecKernelNodeSetParams).
struct StepGraph {
    hipGraphExec_t exec = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphNode_t prep = nullptr;
    std::vector<unsigned char> grad_keep;   // a training graph: per captured step, 1 = the step stores its gradient (step_body's return)
    void release() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        *this = StepGraph();
    }
};

// One form of the training step: its forward launches and their graphs -- one whole step, runs of kMultiSizes[i] steps
// (avae_train_steps), the eval pass.
struct StepPlan {
    std::vector<Launch> fwd;
    StepGraph full, multi[2], eval;
    void release() { full.release(); multi[0].release(); multi[1].release(); eval.release(); }
};

// Device scratch outside the workspace: allocated by the first call that needs it (the workspace does not grow), freed with its
// owner.  Its size is a constant of the handle: another one later is an internal error, not a reallocation.  A first use that
// fails leaves nothing behind, so the next call tries again.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    void* ensure(size_t n, bool zero = false) {
        if (p && n != bytes) throw Err("internal error: device scratch of " + std::to_string(bytes) + " bytes asked for as " + std::to_string(n));
        if (p) return p;
        void* q = nullptr;
        HIP_OK(hipMalloc(&q, n));
        if (zero && hipMemset(q, 0, n) != hipSuccess) { (void)hipFree(q); throw Err("hipMemset of fresh device scratch failed"); }
        p = q; bytes = n;
        return p;
    }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

// The environment switches (A/B runs, diagnostics, tests): read ONCE per handle, by read_switches() at the top of avae_create (and
// of the temporary handles of avae_workspace_bytes / avae_dp_plan), before anything is planned.  Every plan of the handle -- the
// training plan and the serve, inference, masked and completion plans built by a later first call -- follows this copy: a switch
// set or cleared after avae_create does not reach the handle.
struct PlanSwitches {
    // present = on, whatever the value
    bool no_ld_spread = false, no_implicit = false, no_thin = false, no_thin_fast = false, no_adj = false;
    bool no_256 = false, no_32 = false, no_32x32 = false, no_lean = false, no_lean_loss = false, no_lean_head = false, no_64x128 = false,
         no_loss8 = false, no_bias_ep = false, no_bias_mfma = false, no_tn_slices = false, no_tn_balance = false;
    bool no_tail = false, no_wadj_fold = false, no_sink = false, no_sums_merge = false, no_adam_fuse = false, no_xcd_pieces = false,
         no_warm = false, no_desc = false;
    bool chain2 = false, debug_dp = false, comm_no_prio = false;
    // "1" = on
    bool debug_sync = false, plan_dump = false, keep_grads = false;
    // values
    bool tn_g_set = false;
    int tn_g = 1;
    int sched = 0;
    int thin_fast_split[3] = {1, 4, 1};      // measured on c2conv (tools/thin_split_ab.sh): forward 7.1 us at 1 (12.3 at 2, 21.6 at 4), dX 10.4 / 7.6 / 5.8, dF 8.3 / 8.1 / 10.5
    std::string impl_policy = "E:fw,H:fwb,D1:fwb,DT:";
    int ipc_blocks = 256;                    // one workgroup per CU: the exchange is three memory passes over the range, and 64
                                             // workgroups moved them at < 1 TB/s (14 us for C2's 6 MB with one rank, measured)
    double ipc_timeout_ms = 20000.0;         // a peer that is this late has failed: raise the error word instead of hanging
};

struct SwitchRow {
    const char* name;
    bool PlanSwitches::* present;                      // presence-only switches; null: parse() reads the value
    void (*parse)(PlanSwitches&, const char*);
    const char* what;
};
#define AVAE_ONE(member) nullptr, +[](PlanSwitches& s, const char* e) { s.member = e[0] == '1'; }
const SwitchRow kSwitches[] = {
    {"AVAE_NO_LD_SPREAD", &PlanSwitches::no_ld_spread, nullptr, "row strides that are a multiple of 512 bytes stay as they are (spread_ld)"},
    {"AVAE_NO_IMPLICIT", &PlanSwitches::no_implicit, nullptr, "no implicit-GEMM conv route; round 2's compact map layout"},
    {"AVAE_NO_THIN", &PlanSwitches::no_thin, nullptr, "the one-channel stage runs im2col -> GEMM -> col2im, not k_thin"},
    {"AVAE_NO_THIN_FAST", &PlanSwitches::no_thin_fast, nullptr, "k_thin without the block-structured path of the reference's geometry"},
    {"AVAE_NO_ADJ", &PlanSwitches::no_adj, nullptr, "transposed convs keep their fp32 patch gradients (no adjoint-frame route)"},
    {"AVAE_NO_256", &PlanSwitches::no_256, nullptr, "k128x128 where k256x128 would be chosen"},
    {"AVAE_NO_32", &PlanSwitches::no_32, nullptr, "k64x64 where a 32-row tile (and everything lean) would be chosen"},
    {"AVAE_NO_32x32", &PlanSwitches::no_32x32, nullptr, "k32x64 where k32x32 would be chosen"},
    {"AVAE_NO_LEAN", &PlanSwitches::no_lean, nullptr, "no kernel of the k_small family, no k_serve_in, no fused wgrad+adam"},
    {"AVAE_NO_LEAN_LOSS", &PlanSwitches::no_lean_loss, nullptr, "the output + loss launch stays on k32x32"},
    {"AVAE_NO_LEAN_HEAD", &PlanSwitches::no_lean_head, nullptr, "the fused head launches stay on k32x64"},
    {"AVAE_NO_64x128", &PlanSwitches::no_64x128, nullptr, "k128x128 for the wide-latent head launches"},
    {"AVAE_NO_LOSS8", &PlanSwitches::no_loss8, nullptr, "no k256x64Loss; the latent item rides in fwd_out_loss"},
    {"AVAE_NO_BIAS_EP", &PlanSwitches::no_bias_ep, nullptr, "8-wave tiles: the bias row stays in the K loop"},
    {"AVAE_NO_BIAS_MFMA", &PlanSwitches::no_bias_mfma, nullptr, "weight gradients: the bias gradient stays a tile row"},
    {"AVAE_NO_TN_SLICES", &PlanSwitches::no_tn_slices, nullptr, "weight-gradient items are not cut into entries"},
    {"AVAE_NO_TN_BALANCE", &PlanSwitches::no_tn_balance, nullptr, "weight-gradient entries keep plan order over the XCD groups"},
    {"AVAE_NO_TAIL", &PlanSwitches::no_tail, nullptr, "no tail product: fwd_dec1 / bwd_head / serve_dec1 are launches of their own"},
    {"AVAE_NO_WADJ_FOLD", &PlanSwitches::no_wadj_fold, nullptr, "the adjoint filter shadows come from k_wadj, not from k_adam"},
    {"AVAE_NO_SINK", &PlanSwitches::no_sink, nullptr, "mixed models: the MLP modalities' launches stay launches of their own"},
    {"AVAE_NO_SUMS_MERGE", &PlanSwitches::no_sums_merge, nullptr, "column sums, slice sums and k_gperm stay separate launches"},
    {"AVAE_NO_ADAM_FUSE", &PlanSwitches::no_adam_fuse, nullptr, "small nets: k_adam stays a launch of its own"},
    {"AVAE_NO_XCD_PIECES", &PlanSwitches::no_xcd_pieces, nullptr, "wgrad+adam without XCD-owned pieces"},
    {"AVAE_NO_WARM", &PlanSwitches::no_warm, nullptr, "8-wave tiles do not warm the next launch's weight panels"},
    {"AVAE_NO_DESC", &PlanSwitches::no_desc, nullptr, "every launch stays on its by-value arguments (no descriptor table)"},
    {"AVAE_CHAIN2", &PlanSwitches::chain2, nullptr, "experiment: fwd_enc1 + fwd_enc2 of the small nets as one launch (k_chain2)"},
    {"AVAE_DEBUG_DP", &PlanSwitches::debug_dp, nullptr, "say why a data-parallel graph capture fell back"},
    {"AVAE_COMM_NO_PRIO", &PlanSwitches::comm_no_prio, nullptr, "the collective's stream gets no priority"},
    {"AVAE_DEBUG_SYNC", AVAE_ONE(debug_sync), "=1: print and synchronise every launch that runs"},
    {"AVAE_PLAN_DUMP", AVAE_ONE(plan_dump), "=1: serve_plan prints the plan it builds"},
    {"AVAE_KEEP_GRADS", AVAE_ONE(keep_grads), "=1: every fused wgrad+adam launch stores its gradient"},
    {"AVAE_TN_G", nullptr, +[](PlanSwitches& s, const char* e) { s.tn_g_set = true; s.tn_g = std::atoi(e); }, "XCD group of the weight-gradient launches: 1, 2, 4 or 8 (checked by wgrad_entries)"},
    {"AVAE_SCHED", nullptr, +[](PlanSwitches& s, const char* e) { s.sched = std::atoi(e); }, "LaunchArgs::sched of every grouped launch"},
    {"AVAE_THIN_FAST_SPLIT", nullptr, +[](PlanSwitches& s, const char* e) { std::sscanf(e, "%d,%d,%d", &s.thin_fast_split[0], &s.thin_fast_split[1], &s.thin_fast_split[2]); },
     "\"a,b,c\": workgroups per image of the direct stage in mode 0 / 1 / 2"},
    {"AVAE_IMPL_POLICY", nullptr, +[](PlanSwitches& s, const char* e) { s.impl_policy = e; }, "which conv products run as implicit GEMMs (plan_memory)"},
    {"AVAE_IPC_BLOCKS", nullptr, +[](PlanSwitches& s, const char* e) { s.ipc_blocks = std::atoi(e); }, "workgroups of the hipIpc all-reduce (checked by comm_init_ipc)"},
    {"AVAE_IPC_TIMEOUT_MS", nullptr, +[](PlanSwitches& s, const char* e) { s.ipc_timeout_ms = std::atof(e); }, "bound of every wait of the hipIpc all-reduce"},
};
#undef AVAE_ONE

PlanSwitches read_switches() {
    PlanSwitches s;
    for (const SwitchRow& r : kSwitches)
        if (const char* e = std::getenv(r.name)) {
            if (r.present) s.*r.present = true; else r.parse(s, e);
        }
    return s;
}

}  // namespace

struct avae_handle {
    avae_config cfg{};
    std::mutex mu;
    std::string err;
    int es = 2, KU = 64;
    int B = 0, Bp = 0, ldB = 0;   // batch, batch padded to 128 rows, rup(batch, KU)
    int nz = 0, M = 0, ld_eps = 0;
    std::vector<Mod> mods;
    size_t P_flat = 0, P_int = 0, P_enc = 0; // flat API count, internal padded count (floats), floats of the encoder sides (they come first)
    size_t off_theta = 0, off_m = 0, off_v = 0, off_g = 0;   // byte offsets; g has P_int + 64 floats
    size_t stage_lo = 0, stage_bytes = 0;   // input-staging set 0 (X0 / X32 of every modality + eps); sets 1..kMultiSteps-1 follow it
    size_t off_eps = 0, off_partial = 0, off_state = 0, off_items = 0, off_adam = 0, off_inf = 0, off_stamps = 0, off_latent = 0;
    int n_partial = 0;
    size_t ws_bytes = 0;
    unsigned char* ws = nullptr;
    bool own_ws = false;
    hipStream_t cap_stream = nullptr;

    std::vector<WorkItem> items;            // training + eval tables (host mirror)
    std::vector<Launch> bwd;                // training launches (the forward ones are plain.fwd): dgrad chain
    std::vector<Launch> wgrad;              // all weight gradients (-> [all-reduce ->] k_adam)
    std::vector<Launch> wgrad_adam;         // small nets, one replica: the same launch with the Adam step in its epilogue (k_small_tn): no k_adam launch
    // Data-parallel buckets: bucket 0 = the decoder side of every modality (output layer, decoder layers: their weight gradients
    // can be taken as soon as bwd_dec1_latent has run), bucket 1 = the encoder side (heads, encoder layers: after the last dgrad).
    // The all-reduce of bucket 0 runs beside the encoder's dgrad chain and bucket 1's weight gradients; Adam is applied per bucket.
    int n_buckets = 1;                      // 1: models with a conv modality (their helper launches are not bucketed)
    int bwd_split = 0;                      // h->bwd[0 .. bwd_split) belongs to bucket 0's part of the step, the rest to bucket 1's
    std::vector<Launch> wgrad_b[2];
    struct Range { size_t off, count; };    // floats inside the gradient buffer (the cost slot rides at the end of the last range of bucket 0)
    std::vector<Range> ranges_b[2];
    int adam_first_b[2] = {0, 0}, adam_count_b[2] = {0, 0}, adam_blocks_b[2] = {0, 0};   // items of the bucket-ordered copy of the Adam table
    std::vector<AdamItem> adam_items_b;     // [bucket 0 items ..., bucket 1 items ...], tile bases per bucket
    size_t off_adam_b = 0;
    // library-owned collective (RCCL): one communicator per replica, its own stream, events between the two streams
    void* comm = nullptr;                   // AVAE_COMM_RCCL: the ncclComm_t
    int comm_world = 1, comm_rank = 0;
    bool comm_on = false;                   // a library-owned collective (either backend) is up
    size_t off_wire = 0;                    // RCCL with bf16 on the wire: the packed gradient [P_int] bf16
    // AVAE_COMM_IPC: this replica's exchange block (uncached device memory, exported to the peers), the peers' blocks as mapped here
    unsigned char* ipc_block = nullptr;
    size_t ipc_bytes = 0;
    unsigned char* ipc_peer[kMaxWorld] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool ipc_opened[kMaxWorld] = {false, false, false, false, false, false, false, false};
    bool ipc_attached = false;
    IpcArgs ipc_args{};                     // layout + peers; off / granules / cost_idx are filled per call
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_grad[2] = {nullptr, nullptr}, ev_red[2] = {nullptr, nullptr};
    std::vector<StepGraph> g_dp[2];         // per staging set: captured segment of bucket b (forward + backward part + its weight gradients)
    // whole runs of data-parallel steps as ONE graph (staging + per step: segments, all-reduces on the comm stream, Adam per bucket):
    StepGraph g_dpm[2];
    bool dp_graph_failed = false;           // RCCL refused stream capture on this stack: host-stepped pipeline instead
    Launch cost_only;                       // eval: K_COST alone, no step bump
    std::vector<AdamItem> adam_items;
    int adam_blocks = 0;
    // inference tables: per modality, device slots at off_inf
    struct Inf { std::vector<WorkItem> items; std::vector<Launch> launches; int rows = -1; size_t dev_off = 0; };
    std::vector<Inf> inf_enc, inf_dec;
    // serving (avae_generate): per row bucket one staging launch per call + the grouped decoder launches of all modalities (eager
    // after k_serve_in, else one captured graph) with a slot-indirect output move
    struct Serve { int bucket = 0; std::vector<WorkItem> items; std::vector<Launch> launches; hipGraphExec_t graph = nullptr; ServeArgs in;
                   Launch in_launch; bool fused_in = false;
                   ServeInArgs in_lean; int in_lean_grid = 0; bool lean_in = false; };
    std::vector<Serve> serve;
    size_t off_slot = 0;
    // First-use scratch (DevBuf), one allocation per entry point: calls on a handle are ordered on their streams, not exclusive.
    DevBuf iw_buf;                          // avae_loglik: z rows, r, log-weights, running log-sum-exp states of one pass
    DevBuf imp_buf;                         // avae_impute: fused [mu | lv] rows, z rows, r, the running (mean, M2) of one input row
    DevBuf row_pres;                        // masked scoring / impute: the chunk's staged presence bytes [batch_size][M]
    DevBuf topk_buf;                        // avae_latent_topk: the (query, split) lists of one chunk of queries (kTopkScratchBytes)
    DevBuf stats_buf;                       // avae_latent_stats: one partial per (row slice, work item) (kStatsScratchBytes)
    DevBuf agg_buf;                         // avae_agg_logpdf: the (query, slice, column) pairs of one chunk of queries (kAggScratchBytes)
    DevBuf gmm_buf;                         // avae_gmm_fit: one partial per row slice and two parameter sets (kGmmScratchBytes)
    DevBuf embed_buf;                       // avae_embed_*: used bytes, block counts and one partial per (row, split) (kEmbedScratchBytes)
    DevBuf desc_buf;                        // the training plan's per-workgroup descriptors (build_descriptors; Launch::desc_off)
    size_t off_chain = 0;
    size_t off_consts = 0, off_conv_tab = 0;   // 32 B {zeros | one, 0...}; device copy of conv_tab
    std::vector<ConvA> conv_tab;             // implicit patch matrices of the training plan

    // The training step: `plain` (its forward launches are the planner's; graphs captured at create) and, built by the first masked call
    // (avae_train_steps_masked / avae_eval_cost_masked), its masked twin -- the forward launches with WorkItem::present set in their
    // loss and latent items, reading the staged presence bytes (one set of [B][M] per staging set, allocated then: the workspace does
    // not grow).  Backward, weight gradients and Adam are shared.
    StepPlan plain, masked;
    DevBuf pres_buf;
    size_t pres_set = 0;                    // bytes per staging set

    // avae_set_corruption: what the training calls' staging does to the encoder's copy of a modality that came without an explicit
    // input (all zero = off).  Handle state only: not saved, and PrepArgs carry it by value, so enqueued work keeps what it was given.
    avae_corruption corr{};
    unsigned drop_thr[kMaxMod] = {};        // floor(drop_prob * 2^24)

    // avae_set_grad_clip: global-norm clipping / non-finite step skipping.  clip_on switches the step's tail to weight gradients ->
    // k_grad_sumsq -> clip-aware k_adam (never the fused wgrad+adam launch); the threshold and the skip flag live in clip_buf (a
    // ClipState, allocated by the first call that switches clipping on), where the kernels read them.
    bool clip_on = false;
    DevBuf clip_buf;
    long long clip_steps = 0;               // steps submitted since clipping was last switched on (bounds avae_grad_norm_history)

    // avae_set_schedule: KL / association / learning-rate schedules.  sched_on: the training staging launches run their SCHED
    // instance (it fills the step table and the history ring of sched_buf, a SchedState allocated by the first call that switches a
    // schedule on) and the latent and cost items of every training launch carry a pointer to their step's table entry.  The plans'
    // launch tables stay unscheduled -- evaluation and inference run them as they are; run_set patches copies for the training routes.
    bool sched_on = false;
    DevBuf sched_buf;
    long long sched_steps = 0;              // steps submitted since a schedule was last switched on (bounds avae_hyper_history)

    // avae_set_ema: exponential averaging of the parameters.  ema_on: every k_adam launch of a training step runs its EMA instance,
    // which updates the average next to theta (small nets leave the fused weight-gradient + Adam launch, as for clipping); decay
    // and warmup live in the EmaState that leads ema_buf, the average (P_int floats, master layout) behind it -- allocated by the
    // first call that switches averaging on.  averaged (avae_use_averaged): the compute-dtype shadows currently hold the average,
    // not theta -- inference and evaluation run on it, every training call is refused.
    bool ema_on = false, averaged = false;
    float ema_decay = 0.0f;
    int ema_warmup = 0;
    DevBuf ema_buf;

    // avae_complete: the launches of one refinement pass (decoders forward, then their input-gradient chain from the training plan's
    // item builders on the same buffers), captured as runs of kCompleteSizes[i] passes; the kernels' arguments; the scratch behind
    // them.  Built and allocated by the first call.
    struct Complete { bool built = false; std::vector<WorkItem> items; std::vector<Launch> fwd, bwd; CompleteArgs args{};
                      StepGraph g[3]; DevBuf buf; };
    Complete cmpl;

    // Calls on one handle share its activation buffers and serving slot: a call on a different stream than the previous one is
    // ordered behind that one's work (an event recorded on the old stream when the switch is seen: nothing per call otherwise).
    hipStream_t last_stream = nullptr;
    bool has_last_stream = false;
    hipEvent_t ev_switch = nullptr;
    unsigned draw_id = 0;                   // forward-only calls that drew their own eps (next_draw: keys the generator, a fresh draw per call)
    bool timing = false;
    PlanSwitches sw;                        // the environment as avae_create found it
    std::vector<std::string> tnames;
    std::vector<TimingRec> trecs;

    template <typename T> T* at(size_t off) const { return reinterpret_cast<T*>(ws + off); }
    DevState* state() const { return at<DevState>(off_state); }
    float* grad() const { return at<float>(off_g); }
    float* ema_avg() const { return reinterpret_cast<float*>(ema_buf.as<unsigned char>() + sizeof(EmaState)); }
};

namespace {

// Row strides that are a multiple of 512 bytes put the rows of an operand tile (one 128-byte chunk per row and K step) on a
// handful of the L2's address-interleaved channels (a 2048-byte stride: C4's W shadows, 1024 x bf16 -- its dgrad K loop ran
// 1.03 us per tile against 0.90 for the forward's 2176-byte rows).  One more K unit (128 bytes) of zero padding per row avoids it.
// (`spread`: false under AVAE_NO_LD_SPREAD)
inline int spread_ld(int ld, int KU, int es, bool spread) {
    return (spread && ((size_t)ld * es) % 512 == 0) ? ld + KU : ld;
}

Act make_act(Bump& b, int width, bool ones, int rows, int KU, int es, bool spread, int ld = 0) {
    Act a;
    a.width = width;
    a.rows = rows;
    a.ones = ones;
    a.ld = ld > 0 ? ld : spread_ld((int)rup(width + 1, KU), KU, es, spread);       // ld given: a buffer that is never a GEMM operand
    a.rm = b.take(rup(rows, kRowAlign) * (size_t)a.ld * es);
    return a;
}

Dense make_dense(Bump& b, size_t& pint, int in, int out, int KU, int es, bool spread, bool head) {
    Dense d;
    d.in = in; d.out = out; d.head = head;
    d.ld = (int)rup(out, 32);                      // theta / m / v / g rows: whole 128-byte lines (k_adam streams them: rows cut at 16 bytes
                                                   // cost it 9.0 -> 11.75 us on C2), not padded to the K unit.  This layout is what the gradient
                                                   // all-reduce puts on the wire: 6.13 MB for C2's 5.87 MB of parameters (6.6 MB padded to K)
    d.ldw = spread_ld((int)rup(out, KU), KU, es, spread);
    d.ldt = spread_ld((int)rup(in + 1, KU), KU, es, spread);
    d.master = pint;
    pint += (size_t)(in + 1) * d.ld;
    d.W = b.take(rup(in + 1, kRowAlign) * (size_t)d.ldw * es);
    d.Wt = b.take(rup(out, kRowAlign) * (size_t)d.ldt * es);
    return d;
}

void check_config(const avae_config& c) {
    if (c.abi_version != AVAE_ABI_VERSION) throw Err("avae_config.abi_version mismatch");
    if (c.n_modalities < 1 || c.n_modalities > AVAE_MAX_MODALITIES) throw Err("n_modalities out of range");
    if (c.n_z < 1 || c.n_z > 64) throw Err("n_z must be in [1,64] (the fused head/latent epilogue holds 2*n_z columns in one tile)");
    if (c.batch_size < 1) throw Err("batch_size must be positive");
    if (c.compute_dtype != AVAE_F32 && c.compute_dtype != AVAE_BF16) throw Err("compute_dtype must be AVAE_F32 or AVAE_BF16");
    if (c.activation < AVAE_ACT_IDENTITY || c.activation > AVAE_ACT_TANH) throw Err("unknown activation");
    if (c.comm_buckets != 0 && c.comm_buckets != 1 && c.comm_buckets != 2) throw Err("comm_buckets must be 0, 1 or 2");
    if (c.wire_dtype != AVAE_F32 && c.wire_dtype != AVAE_BF16) throw Err("wire_dtype must be AVAE_F32 or AVAE_BF16");
    if (c.use_comm < AVAE_COMM_NONE || c.use_comm > AVAE_COMM_IPC) throw Err("use_comm must be AVAE_COMM_NONE, AVAE_COMM_RCCL or AVAE_COMM_IPC");
    for (int m = 0; m < c.n_modalities; ++m) {
        const avae_modality& mo = c.mod[m];
        if (mo.n_input < 1) throw Err("n_input must be positive");
        if (mo.hidden_conv) {
            // the reference's branch is hard-wired to 28x28: 28 -> 14 -> 7 -> 3 in the encoder (vae_assoc.py:171-199),
            // 1 -> 3 -> 7 -> 14 -> 28 in the decoder (:250-278) and a dense n_input x n_input on top (:287)
            if (mo.n_input != 784) throw Err("hidden_conv needs n_input = 784 (28x28 images)");
            if (!mo.binary) throw Err("hidden_conv needs a binary modality (the reference's non-binary conv decoder is shape-broken, vae_assoc.py:299)");
            if (mo.n_hidden_layers != 2 || mo.conv_gener[0] < 2 || mo.conv_gener[1] < 1) throw Err("hidden_conv needs n_hidden_recog_1/2 and n_hidden_gener_1 (>=2) / n_hidden_gener_2");
        }
        if (mo.n_hidden_layers < 1 || mo.n_hidden_layers > AVAE_MAX_HIDDEN) throw Err("n_hidden_layers out of range");
        for (int k = 0; k < mo.n_hidden_layers; ++k)
            if (mo.n_hidden[k] < 1) throw Err("hidden width must be positive");
    }
}

// Lays out the whole workspace; with h->ws == nullptr it only computes sizes.
// workgroups per image of the direct one-channel stage: 1 on the block-structured path (the reference's geometry), else kThinSplit
inline bool thin_fast(const PlanSwitches& sw, const ConvGeom& g) { return thin_fast_geometry(g) && !sw.no_thin_fast; }
// workgroups per image of the direct one-channel stage in mode 0 / 1 / 2 (AVAE_THIN_FAST_SPLIT="a,b,c": A/B runs)
inline int thin_split(const PlanSwitches& sw, const ConvGeom& g, int mode) {
    if (!thin_fast(sw, g)) return kThinSplit;
    const int v = sw.thin_fast_split[mode];
    return v == 1 || v == 2 || v == 4 ? v : 1;
}

void plan_memory(avae_handle* h) {
    const avae_config& c = h->cfg;
    h->es = c.compute_dtype == AVAE_BF16 ? 2 : 4;
    h->KU = kTileBytesK / h->es;
    h->B = c.batch_size;
    h->Bp = (int)rup(h->B, kRowAlign);
    h->ldB = (int)rup(h->B, h->KU);
    h->nz = c.n_z;
    h->ld_eps = (int)rup(c.n_z, 4);
    h->M = c.n_modalities;
    const int KU = h->KU, es = h->es, Bp = h->Bp, ldB = h->ldB, nz = h->nz, B = h->B;
    const PlanSwitches& sw = h->sw;
    const bool spread = !sw.no_ld_spread;
    Bump b;
    size_t pint = 0, pflat = 0;
    h->mods.clear();
    // Input staging first, as one contiguous block, followed by kMultiSteps-1 more copies of it: the multi-step graph
    // stages all its batches with one launch and step j of a replay reads set j (build_training_plan relocates the
    // pointers); every other path uses set 0.
    std::vector<Act> stage_x0(h->M);
    std::vector<size_t> stage_x32(h->M);
    h->stage_lo = b.off;
    for (int m = 0; m < h->M; ++m) {
        const avae_modality& mo = c.mod[m];
        stage_x0[m] = make_act(b, mo.n_input, mo.hidden_conv == 0, B, KU, es, spread);
        stage_x32[m] = b.take((size_t)B * rup(mo.n_input, 8) * 4);
    }
    h->off_eps = b.take((size_t)B * h->ld_eps * 4);
    h->stage_bytes = b.off - h->stage_lo;
    b.take(h->stage_bytes * (kMultiSteps - 1));
    for (int m = 0; m < h->M; ++m) {
        const avae_modality& mo = c.mod[m];
        Mod md;
        md.n_in = mo.n_input;
        md.L = mo.n_hidden_layers;
        md.hs.assign(mo.n_hidden, mo.n_hidden + md.L);
        md.conv = mo.hidden_conv != 0;
        auto act_B = [&](int width, bool ones) { return make_act(b, width, ones, B, KU, es, spread); };
        if (!md.conv) {
            int prev = md.n_in;
            for (int k = 0; k < md.L; ++k) { md.enc.push_back(make_dense(b, pint, prev, md.hs[k], KU, es, spread, false)); pflat += (size_t)(prev + 1) * md.hs[k]; prev = md.hs[k]; }
            md.head = make_dense(b, pint, prev, 2 * nz, KU, es, spread, true);
            pflat += (size_t)(prev + 1) * 2 * nz;
            prev = nz;
            for (int k = 0; k < md.L; ++k) { md.dec.push_back(make_dense(b, pint, prev, md.hs[k], KU, es, spread, false)); pflat += (size_t)(prev + 1) * md.hs[k]; prev = md.hs[k]; }
            md.outl = make_dense(b, pint, prev, md.n_in, KU, es, spread, false);
            pflat += (size_t)(prev + 1) * md.n_in;
            md.X0 = stage_x0[m];
            for (int k = 0; k < md.L; ++k) md.E.push_back(act_B(md.hs[k], true));
            md.Z = act_B(nz, true);
            for (int k = 0; k < md.L; ++k) md.D.push_back(act_B(md.hs[k], true));
            for (int k = 0; k < md.L; ++k) md.dE.push_back(act_B(md.hs[k], false));
            md.dH = act_B(2 * nz, false);
            for (int k = 0; k < md.L; ++k) md.dD.push_back(act_B(md.hs[k], false));
            md.dO = act_B(md.n_in, false);
        } else {
            const int R1 = md.hs[0], R2 = md.hs[1], G1 = mo.conv_gener[0], G2 = mo.conv_gener[1];
            md.L = 0;
            md.X0 = stage_x0[m];
            md.Z = act_B(nz, false);
            md.dH = act_B(2 * nz, false);
            md.dO = act_B(md.n_in, false);
            const bool no_impl = sw.no_implicit;
            auto stage = [&](int IH, int Cin_in, int OH, int Cout, int k, int so, int d, int pad, bool bias, int act, int flat, bool plain_out, bool has_dgrad) {
                ConvStage st;
                // whole 16-byte chunks of channels per tap where that takes a few zero channels (the first decoder stage reads z: n_z
                // channels, padded here; the pad channels' filter rows stay zero and are not part of the flat parameters)
                const int cpc = 16 / es;
                const int Cin = (IH == 1 && flat == 1 && !no_impl) ? (int)rup(Cin_in, cpc) : Cin_in;
                st.cin_real = Cin_in;
                st.g = ConvGeom{B, IH, IH, Cin, OH, OH, k, so, d, pad, 0, 0, bias ? 1 : 0};
                st.bias = bias; st.act = act; st.flat = flat;
                const int K = k * k * Cin, rows = B * OH * OH;
                st.d = make_dense(b, pint, K, Cout, KU, es, spread, flat == 3);
                st.P = make_act(b, K, bias, rows, KU, es, spread);
                const bool thin = Cout == 1 && plain_out && flat == 1 && IH > 1 && IH * IH * Cin <= kThinIn && OH * OH <= kThinOut && K + 1 <= kThinF && !sw.no_thin;
                // (the dense layer behind the flattened 28x28 map, flat == 2, is never a conv: it reads the map as stored -- dense_map -- or its flatten gather)
                // (row -> (image, pixel) by magic-number division: exact while rows x pixels-per-image < 2^32)
                const bool fits = (uint64_t)rows * (uint64_t)(OH * OH) < (1ull << 32) && (uint64_t)B * IH * IH * (uint64_t)(IH * IH) < (1ull << 32);
                {   // Which products of which stage run as implicit GEMMs.  The gather is dense in the conv direction (big map -> small
                    // map: every tap of every row is a real pixel) and mostly zeros in the transposed direction (zero insertion / full
                    // padding: 3 of 4 taps of a stride-2 transposed conv read the zero block), where the scatter product on the small
                    // side (round 2's adjoint-frame route) or the explicit patch gradients do a quarter of the work.  Measured on c2conv
                    // (tools/conv_policy_ab.sh, one box, ms per step): everything explicit 0.2715; everything implicit 0.2696 (22
                    // launches: conv forward 7.3 us vs 8.2 + 4.4, heads 7.5 vs 4.2 + 5.3, first decoder stage 4.2 vs 4.3 + 4.4, its
                    // latent dgrad 6.8 vs 4.5 + 6.0 -- but transposed-conv forward 24.3 vs 11.7 + 7.2, conv dgrad 23.6 vs 10.4 + 6.6,
                    // gather-form filter gradients 43 vs 17); implicit where the gather is dense 0.2376 (29 launches) = the default:
                    //   E  conv stages        forward + filter gradient implicit, input gradient by patch gradients + col2im
                    //   H  heads, D1 first decoder stage (1x1 input)   everything implicit
                    //   DT transposed convs   round 2's adjoint-frame route (scatter product + overlap-add, Padj for both gradients);
                    //                         their implicit input gradient alone ("DT:b": 8.3 us vs 5.9 with Padj at hand) 0.2436
                    // Letters f / w / b = forward / filter gradient / input gradient; AVAE_IMPL_POLICY overrides (A/B runs, tests).
                    const std::string& policy = sw.impl_policy;      // (default "E:fw,H:fwb,D1:fwb,DT:")
                    const std::string cls = flat == 0 ? "E" : flat == 3 ? "H" : (flat == 1 && IH == 1) ? "D1" : flat == 1 ? "DT" : "X";
                    std::string letters;
                    for (size_t pos = 0; pos < policy.size();) {
                        const size_t e = policy.find(',', pos), c = policy.find(':', pos);
                        const size_t end = e == std::string::npos ? policy.size() : e;
                        if (c != std::string::npos && c < end && policy.substr(pos, c - pos) == cls) letters = policy.substr(c + 1, end - c - 1);
                        pos = end + 1;
                    }
                    const bool geo = !no_impl && fits && !thin && flat != 2 && (so == 1 || so == 2) && (d == 1 || d == 2);
                    st.impl = geo && letters.find('f') != std::string::npos && (Cin * es) % 16 == 0;
                    st.impl_w = geo && (st.impl || letters.find('w') != std::string::npos) && (Cin * es) % 16 == 0;
                    st.impl_bwd = geo && letters.find('b') != std::string::npos && has_dgrad && (Cout * es) % 16 == 0;
                    // Wide latents (2 n_z > 64): the head and latent-dgrad launches run on the 128-column tiles, which carry no
                    // gather -- the heads' forward and the first decoder stage's latent gradient stay on their explicit routes there
                    // (tools/fuzz_parity.py found the planner throwing for n_z = 33 with a conv modality).
                    if (2 * h->nz > 64) {
                        if (cls == "H") st.impl = false;
                        if (cls == "D1") st.impl_bwd = false;
                    }
                }
                if (plain_out) {     // hidden conv stage: own output / gradient buffers
                    // (the direct stage's one-channel maps are read and written pixel by pixel: the LAST map (28x28), whose consumer
                    // is the dense output layer, is stored as dense rows [B][784 | 1]: that layer then reads it as any dense layer
                    // reads its input.  AVAE_NO_IMPLICIT keeps round 2's compact 8-elements-per-pixel layout + flatten gather.)
                    st.dense_map = thin && OH == 28 && !no_impl;
                    if (st.dense_map) {
                        st.Y = make_act(b, OH * OH, true, B, KU, es, spread);
                        st.dY = make_act(b, OH * OH, false, B, KU, es, spread);
                    } else {
                        const int compact = thin && OH == 28 ? 8 : 0;
                        st.Y = make_act(b, Cout, false, rows, KU, es, spread, compact);
                        st.dY = make_act(b, Cout, false, rows, KU, es, spread, compact);
                    }
                }
                st.lddp = (int)rup(K, 8);
                st.dP = b.take((size_t)rows * st.lddp * 4);
                {   // a conv stage's weight gradient sums over batch x output pixels (up to 200 704 rows) into a few tiles:
                    // cut that K range so that the launch has a few hundred workgroups of at least 8 K tiles each
                    const int steps = (int)(rup(rows, KU) / KU), tiles = ((K + 1 + 63) / 64) * ((Cout + 63) / 64);
                    int split = std::min(steps / 8, (512 + tiles - 1) / tiles);
                    if (split > 1) {
                        st.kchunk = (steps + split - 1) / split;
                        st.ksplit = (steps + st.kchunk - 1) / st.kchunk;
                        st.part = b.take((size_t)st.ksplit * (K + 1) * st.d.ld * 4);
                    }
                }
                // transposed convs that upsample (d > 1) or pad heavily have an OUTPUT far larger than their input: the fp32 patch
                // gradients [B*OH*OW][k*k*Cin] of the plain path (160 MB for 7x7x32 -> 14x14x16) are replaced by the compute-type
                // patch matrix of the output gradient, [B*IH*IW][k*k*Cout] (11 MB), times the adjoint filter
                if (flat == 1 && plain_out && !thin && !st.impl && IH > 1 && Cout <= 64 && (long)IH * IH * Cout < (long)OH * OH * Cin * 2 && !sw.no_adj) {
                    st.adj = true;
                    st.Padj = make_act(b, k * k * Cout, false, B * IH * IH, KU, es, spread);
                    st.ldadj = (int)rup(k * k * Cout, KU);
                    st.Wadj = b.take(rup(Cin, kRowAlign) * (size_t)st.ldadj * es);
                    const int KA = k * k * Cout, rin = B * IH * IH;
                    st.ldf = (int)rup(Cin, KU);
                    st.Wf = b.take(rup(KA, kRowAlign) * (size_t)st.ldf * es);
                    st.ldT = (int)rup(KA, 8);
                    st.T = b.take((size_t)rin * st.ldT * 4);
                    st.ldga = (int)rup(KA, 4);
                    st.Gadj = b.take((size_t)Cin * st.ldga * 4);
                    {   // split of the adjoint filter gradient's K range (= input pixels), as for the plain stages above
                        const int steps = (int)(rup(rin, KU) / KU), tiles = ((Cin + 63) / 64) * ((KA + 63) / 64);
                        const int split = std::min(steps / 8, (512 + tiles - 1) / tiles);
                        if (split > 1) {
                            st.akchunk = (steps + split - 1) / split;
                            st.aksplit = (steps + st.akchunk - 1) / st.akchunk;
                            st.apart = b.take((size_t)st.aksplit * Cin * st.ldga * 4);
                        }
                    }
                    st.rs_cols4 = (int)rup(Cout, 4);
                    st.rs_part = b.take((size_t)kRowsumBlocks * st.rs_cols4 * 4);
                }
                if (st.impl_bwd && !st.Wadj) {      // adjoint filter shadow [Cin][(kh', kw', co)]: the B operand of the implicit input gradient
                    st.ldadj = (int)rup(k * k * Cout, KU);
                    st.Wadj = b.take(rup(Cin, kRowAlign) * (size_t)st.ldadj * es);
                }
                if (thin) {
                    st.thin = true;
                    st.thin_kp = (int)rup(K + 1, 4);
                    st.thin_blocks = B * thin_split(sw, st.g, 2);      // filter-gradient partial sums: one slice per workgroup
                    st.thin_part = b.take((size_t)st.thin_blocks * st.thin_kp * 4);
                }
                pflat += (size_t)k * k * Cin_in * Cout + (flat == 0 ? 0 : Cout);
                return st;
            };
            // encoder: conv k5 s2 SAME (pad-before 1), conv k5 s2 SAME, conv k5 s1 VALID, flatten(3x3) + dense heads
            md.cenc.push_back(stage(28, 1, 14, R1, 5, 2, 1, 1, false, AVAE_ACT_IDENTITY, 0, true, false));
            md.cenc.push_back(stage(14, R1, 7, 2 * R1, 5, 2, 1, 1, false, AVAE_ACT_IDENTITY, 0, true, true));
            md.cenc.push_back(stage(7, 2 * R1, 3, R2, 5, 1, 1, 0, false, AVAE_ACT_IDENTITY, 0, true, true));
            md.cenc.push_back(stage(3, R2, 1, 2 * nz, 3, 1, 1, 0, true, AVAE_ACT_IDENTITY, 3, false, true));
            // decoder: transposed convs as convs of the dilated input with the flipped filter (pad = k-1-pad_before)
            md.cdec.push_back(stage(1, nz, 3, G1, 3, 1, 1, 2, true, AVAE_ACT_SIGMOID, 1, true, true));
            md.cdec.push_back(stage(3, G1, 7, G1 / 2, 5, 1, 1, 4, true, AVAE_ACT_SIGMOID, 1, true, true));
            md.cdec.push_back(stage(7, G1 / 2, 14, G2, 5, 1, 2, 3, true, AVAE_ACT_SIGMOID, 1, true, true));
            md.cdec.push_back(stage(14, G2, 28, 1, 5, 1, 2, 3, true, AVAE_ACT_SIGMOID, 1, true, true));
            md.cdec.push_back(stage(28, 1, 1, md.n_in, 28, 1, 1, 0, true, AVAE_ACT_IDENTITY, 2, false, true));
            md.head = md.cenc[3].d;
            md.outl = md.cdec[4].d;
            auto src = [](ConvStage& st, int sb, int sp) { st.g.src_sb = sb; st.g.src_sp = sp; };
            src(md.cenc[0], md.X0.ld, 1);
            for (int i = 1; i < 4; ++i) { const ConvStage& pv = md.cenc[i - 1]; src(md.cenc[i], pv.g.OH * pv.g.OW * pv.Y.ld, pv.Y.ld); }
            src(md.cdec[0], md.Z.ld, 0);
            for (int i = 1; i < 5; ++i) {
                const ConvStage& pv = md.cdec[i - 1];
                if (pv.dense_map) src(md.cdec[i], pv.Y.ld, 1);        // one channel, dense rows: image stride = row stride, pixel stride 1
                else src(md.cdec[i], pv.g.OH * pv.g.OW * pv.Y.ld, pv.Y.ld);
            }
        }
        md.ld32 = (int)rup(md.n_in, 8);      // multiple of the widest epilogue vector (8 elements)
        md.X32 = stage_x32[m];
        md.out32 = b.take((size_t)B * md.ld32 * 4);
        md.mulv = b.take((size_t)B * 2 * nz * 4);
        md.g0 = b.take((size_t)B * 3 * h->ld_eps * 4);  // [g0mu | g0lv | dz/dlv factor], each roundup(n_z, 4) wide
        h->mods.push_back(std::move(md));
    }
    // Master layout (theta, m, v, g share it): the ENCODER side of every modality first, then every DECODER side, the step's cost in
    // the float right behind -- so each data-parallel bucket is ONE contiguous float range (bucket 1 = [0, P_enc), bucket 0 =
    // [P_enc, P_int + 1)) and the whole buffer one range.  The flat API order (reference creation order) is untouched: it is
    // mapped through Dense::master.
    {
        size_t pm = 0;
        auto place = [&](Dense& d) { d.master = pm; pm += (size_t)(d.in + 1) * d.ld; };
        for (Mod& md : h->mods) {
            if (md.conv) { for (ConvStage& st : md.cenc) place(st.d); md.head = md.cenc[3].d; }
            else { for (Dense& d : md.enc) place(d); place(md.head); }
        }
        h->P_enc = pm;
        for (Mod& md : h->mods) {
            if (md.conv) { for (ConvStage& st : md.cdec) place(st.d); md.outl = md.cdec[4].d; }
            else { for (Dense& d : md.dec) place(d); place(md.outl); }
        }
        if (pm != pint) throw Err("internal error: master layout size");
    }
    h->P_int = pint;
    h->P_flat = pflat;
    h->off_theta = b.take(pint * 4);
    h->off_m = b.take(pint * 4);
    h->off_v = b.take(pint * 4);
    h->off_g = b.take((pint + 64) * 4);      // + cost slot (element P_int), padded
    if (c.use_comm == AVAE_COMM_RCCL && c.wire_dtype == AVAE_BF16) h->off_wire = b.take((pint + 64) * 2);     // the gradient as it travels
    // cost partial slots: one per output-loss tile (the smallest tile, 32x32, bounds the count) + latent tiles
    int slots = (B + kLatentRows - 1) / kLatentRows;
    for (int m = 0; m < h->M; ++m) slots += ((B + 31) / 32) * ((h->mods[m].n_in + 31) / 32);
    h->n_partial = slots;
    h->off_partial = b.take((size_t)slots * 4);
    h->off_state = b.take(sizeof(DevState));
    // work-item tables: training items + eval cost item; inference tables per modality
    size_t n_train_items = 0;
    for (int m = 0; m < h->M; ++m) n_train_items += 6 * (size_t)h->mods[m].L + 8;
    n_train_items += 8;
    h->off_items = b.take(n_train_items * sizeof(WorkItem));
    size_t n_adam = 0;
    for (int m = 0; m < h->M; ++m) n_adam += h->mods[m].conv ? 9 : 2 * (size_t)h->mods[m].L + 2;
    h->off_adam = b.take(n_adam * sizeof(AdamItem));
    h->off_adam_b = b.take(n_adam * sizeof(AdamItem));
    h->off_slot = b.take(sizeof(ServeSlot));
    h->off_consts = b.take(32);
    h->off_chain = b.take((kMaxMod * 64 + 1) * 4);      // k_chain2: a ticket counter per (modality, row block), + its error word
    h->off_conv_tab = b.take(4 * kMaxConvA * kMaxMod * sizeof(ConvA));
    h->off_inf = b.off;
    for (int m = 0; m < h->M; ++m) b.take(2 * ((size_t)h->mods[m].L + 1) * sizeof(WorkItem));
#ifdef AVAE_STAMPS
    h->off_stamps = b.take((size_t)kStampLaunches * kStampBlocks * kStampWords * 8);
#endif
    h->ws_bytes = b.off;
}

// ----------------------------------------------------------------------------- flat <-> internal
template <bool ToInternal>
void convert_params(const avae_handle* h, float* flat, float* internal) {
    size_t f = 0;
    auto dense = [&](const Dense& d) {
        float* I = internal + d.master;
        if (!d.head) {
            for (int r = 0; r < d.in; ++r)
                for (int c = 0; c < d.out; ++c, ++f) { if (ToInternal) I[(size_t)r * d.ld + c] = flat[f]; else flat[f] = I[(size_t)r * d.ld + c]; }
            for (int c = 0; c < d.out; ++c, ++f) { if (ToInternal) I[(size_t)d.in * d.ld + c] = flat[f]; else flat[f] = I[(size_t)d.in * d.ld + c]; }
        } else {
            const int nz = d.out / 2;
            for (int half = 0; half < 2; ++half) {
                for (int r = 0; r < d.in; ++r)
                    for (int c = 0; c < nz; ++c, ++f) { float& x = I[(size_t)r * d.ld + half * nz + c]; if (ToInternal) x = flat[f]; else flat[f] = x; }
                for (int c = 0; c < nz; ++c, ++f) { float& x = I[(size_t)d.in * d.ld + half * nz + c]; if (ToInternal) x = flat[f]; else flat[f] = x; }
            }
        }
    };
    auto xfer = [&](float& x) { if (ToInternal) x = flat[f]; else flat[f] = x; ++f; };
    auto conv_stage = [&](const ConvStage& st) {
        const Dense& d = st.d;
        float* I = internal + d.master;
        const int k = st.g.k, Ci = st.g.Cin, Co = d.out, K = k * k * Ci;
        if (st.flat == 0) {            // tf.nn.conv2d filter [k,k,ci,co] == matrix rows (kh,kw,ci) x cols co; no bias
            for (int r = 0; r < K; ++r) for (int c = 0; c < Co; ++c) xfer(I[(size_t)r * d.ld + c]);
        } else if (st.flat == 1) {     // conv2d_transpose filter [k,k,co,ci] (deconv.py:78), flipped into the matrix; bias[co]
            // (ci runs over the reference's channels; a stage whose input is padded to whole chunks keeps zero rows for the pads)
            for (int kh = 0; kh < k; ++kh) for (int kw = 0; kw < k; ++kw) for (int co = 0; co < Co; ++co) for (int ci = 0; ci < st.cin_real; ++ci)
                xfer(I[(size_t)(((k - 1 - kh) * k + (k - 1 - kw)) * Ci + ci) * d.ld + co]);
            for (int co = 0; co < Co; ++co) xfer(I[(size_t)K * d.ld + co]);
        } else {
            dense(d);                  // dense on the flattened map (2) or the fused heads (3: d.head)
        }
    };
    for (const Mod& md : h->mods) {
        if (md.conv) {
            for (const ConvStage& st : md.cenc) conv_stage(st);
            for (const ConvStage& st : md.cdec) conv_stage(st);
            continue;
        }
        for (const Dense& d : md.enc) dense(d);
        dense(md.head);
        for (const Dense& d : md.dec) dense(d);
        dense(md.outl);
    }
    if (f != h->P_flat) throw Err("internal error: flat parameter count mismatch");
}

// ----------------------------------------------------------------------------- work items
WorkItem gemm_item(int kind, int M, int N, int K, const void* A, int lda, const void* B, int ldb) {
    WorkItem w;
    std::memset(&w, 0, sizeof(w));
    w.kind = kind; w.M = M; w.N = N; w.K = K; w.A = A; w.lda = lda; w.B = B; w.ldb = ldb;
    return w;
}

struct Builder {
    avae_handle* h;
    std::vector<WorkItem>& items;
    int B;      // rows of this plan (batch or inference rows)
    bool train; // training plan (losses, gradients) or inference plan
    int next_slot = 0;
    Builder(avae_handle* h_, std::vector<WorkItem>& it, int rows, bool tr) : h(h_), items(it), B(rows), train(tr) {}
    template <typename T> T* p(size_t off) const { return h->at<T>(off); }
    int K_of(int n) const { return (int)rup(n, h->KU); }

    WorkItem fwd_hidden(const Act& in, const Dense& d, const Act& out) {
        WorkItem w = gemm_item(K_FWD_HIDDEN, B, d.out, K_of(d.in + 1), p<void>(in.rm), in.ld, p<void>(d.Wt), d.ldt);
        w.act = h->cfg.activation;
        w.out0 = p<void>(out.rm); w.ld0 = out.ld;
        w.kin = d.in; w.aux1 = p<unsigned char>(d.W) + (size_t)d.in * d.ldw * h->es; w.ld1 = d.ldw;   // bias row (see WorkItem::bias_ep)
        return w;
    }
    WorkItem fwd_head(const Mod& md, bool with_z, bool implicit = false) {
        const Act& in = md.conv ? md.cenc[3].P : md.E.back();
        WorkItem w = gemm_item(K_FWD_HEAD, B, 2 * h->nz, K_of(md.head.in + 1), p<void>(in.rm), in.ld, p<void>(md.head.Wt), md.head.ldt);
        if (implicit) {          // conv encoder: the flattened 3x3 map, gathered by the GEMM itself
            ConvGeom g = md.cenc[3].g; g.B = B;
            w.A = p<void>(h->off_consts); w.lda = 0;
            w.conv = add_conv(g, p<void>(md.cenc[2].Y.rm), true);
        }
        w.nz = h->nz;
        w.out0 = p<void>(md.mulv); w.ld0 = 2 * h->nz;
        w.out1 = with_z ? p<void>(md.Z.rm) : nullptr; w.ld1 = md.Z.ld;
        w.aux0 = p<void>(h->off_eps); w.ldx = h->ld_eps;
        return w;
    }
    WorkItem fwd_out(const Mod& md, int m, bool loss) {
        const Act& in = md.conv ? (md.cdec[3].dense_map ? md.cdec[3].Y : md.cdec[4].P) : md.D.back();
        WorkItem w = gemm_item(loss ? K_FWD_OUT_LOSS : K_FWD_OUT_STORE, B, md.n_in, K_of(md.outl.in + 1), p<void>(in.rm), in.ld,
                               p<void>(md.outl.Wt), md.outl.ldt);
        w.binary = h->cfg.mod[m].binary ? 1 : 0;
        if (loss && !md.conv) { w.kin = md.outl.in; w.aux1 = p<unsigned char>(md.outl.W) + (size_t)md.outl.in * md.outl.ldw * h->es; w.ld1 = md.outl.ldw; }
        const float bg = (float)(h->cfg.batch_global > 0 ? h->cfg.batch_global : h->cfg.batch_size);
        if (loss) {
            w.scale = w.binary ? h->cfg.mod[m].weight / bg : h->cfg.mod[m].weight;
            w.aux0 = p<void>(md.X32); w.ldx = md.ld32;
            w.out0 = p<void>(md.dO.rm); w.ld0 = md.dO.ld;
            w.partial = p<float>(h->off_partial);
        } else {
            w.out0 = p<void>(md.out32); w.ld0 = md.ld32;
        }
        return w;
    }
    WorkItem dgrad_hidden(const Act& dA, const Dense& d, const Act& yprev, const Act& dprev) {
        WorkItem w = gemm_item(K_DGRAD_HIDDEN, B, d.in, K_of(d.out), p<void>(dA.rm), dA.ld, p<void>(d.W), d.ldw);
        w.act = h->cfg.activation;
        w.aux0 = p<void>(yprev.rm); w.ldx = yprev.ld;
        w.out0 = p<void>(dprev.rm); w.ld0 = dprev.ld;
        return w;
    }
    WorkItem dgrad_latent(const Mod& md) {
        const Dense& d = md.dec[0];
        const Act& dA = md.dD[0];
        WorkItem w = gemm_item(K_DGRAD_LATENT, B, h->nz, K_of(d.out), p<void>(dA.rm), dA.ld, p<void>(d.W), d.ldw);
        w.nz = h->nz;
        w.aux2 = p<void>(md.g0);
        w.out0 = p<void>(md.dH.rm); w.ld0 = md.dH.ld;
        return w;
    }
    // ---- conv branch: every stage is a GEMM on its patch matrix
    int conv_rows(const ConvStage& st) const { return B * st.g.OH * st.g.OW; }
    WorkItem conv_fwd(const ConvStage& st) {
        WorkItem w = gemm_item(K_FWD_HIDDEN, conv_rows(st), st.d.out, K_of(st.d.in + 1), p<void>(st.P.rm), st.P.ld, p<void>(st.d.Wt), st.d.ldt);
        w.act = st.act;
        w.out0 = p<void>(st.Y.rm); w.ld0 = st.Y.ld;
        return w;
    }
    WorkItem conv_dgrad(const ConvStage& st, const Act& dA) {          // fp32 patch gradients dP = dA . W^T
        WorkItem w = gemm_item(K_DGRAD_F32, conv_rows(st), st.d.in, K_of(st.d.out), p<void>(dA.rm), dA.ld, p<void>(st.d.W), st.d.ldw);
        w.out0 = p<void>(st.dP); w.ld0 = st.lddp;
        return w;
    }
    // input gradient of a transposed-conv stage through the adjoint patch matrix (ConvStage::adj)
    GatherSeg adj_gather_seg(const ConvStage& st) {
        GatherSeg g;
        std::memset(&g, 0, sizeof(g));
        const ConvGeom& f = st.g;
        // rows = the stage's input pixels, columns = (kh', kw', co) with kh' = k-1-kh: source row oh = (ih*d + kh' - (k-1-pad))/so
        g.g = ConvGeom{B, f.OH, f.OW, st.d.out, f.IH, f.IW, f.k, f.d, f.so, f.k - 1 - f.pad, f.OH * f.OW * st.dY.ld, st.dY.ld, 0};
        g.src = p<void>(st.dY.rm);
        g.P = p<void>(st.Padj.rm); g.ldp = st.Padj.ld;
        tile_shape(B * f.IH * f.IW, f.k * f.k * st.d.out, &g.cl, &g.rpt, &g.tiles_r, &g.tiles_c);
        return g;
    }
    // forward of such a stage: T = X . Wadj (rows = its input pixels), then overlap-add + bias + transfer function
    WorkItem adj_fwd(const ConvStage& st, const ConvStage& prev) {
        const int rows = B * st.g.IH * st.g.IW, KA = st.g.k * st.g.k * st.d.out;
        WorkItem w = gemm_item(K_DGRAD_F32, rows, KA, K_of(st.g.Cin), p<void>(prev.Y.rm), prev.Y.ld, p<void>(st.Wf), st.ldf);
        w.out0 = p<void>(st.T); w.ld0 = st.ldT;
        return w;
    }
    Col2imSeg adj_overlap_seg(const ConvStage& st) {
        Col2imSeg c;
        std::memset(&c, 0, sizeof(c));
        const ConvGeom& f = st.g;
        c.g = ConvGeom{B, f.OH, f.OW, st.d.out, f.IH, f.IW, f.k, f.d, f.so, f.k - 1 - f.pad, 0, 0, 0};
        c.dP = p<float>(st.T); c.lddp = st.ldT;
        c.bias = p<unsigned char>(st.d.Wt) + (size_t)st.d.in * h->es; c.bias_ld = st.d.ldt;
        c.act = st.act;
        c.dA = p<void>(st.Y.rm); c.lda = st.Y.ld;
        tile_shape(B * f.OH * f.OW, st.d.out, &c.cl, &c.rpt, &c.tiles_r, &c.tiles_c);
        return c;
    }
    // filter gradient in the adjoint frame: Gadj[ci][(kh', kw', co)] = sum over input pixels of X[p][ci] * Padj[p][...]
    WorkItem adj_wgrad(const ConvStage& st, const ConvStage& prev) {
        const int rows = B * st.g.IH * st.g.IW, KA = st.g.k * st.g.k * st.d.out;
        WorkItem w = gemm_item(K_WGRAD, st.g.Cin, KA, K_of(rows), p<void>(prev.Y.rm), prev.Y.ld, p<void>(st.Padj.rm), st.Padj.ld);
        w.out0 = p<void>(st.Gadj); w.ld0 = st.ldga;
        if (st.aksplit > 1) { w.ksplit = st.aksplit; w.kchunk = st.akchunk; w.out1 = p<void>(st.apart); }
        w.bias_row = -1;
        return w;
    }
    WorkItem adj_dgrad(const ConvStage& st, const ConvStage& prev) {
        const int rows = B * st.g.IH * st.g.IW, KA = st.g.k * st.g.k * st.d.out;
        WorkItem w = gemm_item(K_DGRAD_HIDDEN, rows, st.g.Cin, K_of(KA), p<void>(st.Padj.rm), st.Padj.ld, p<void>(st.Wadj), st.ldadj);
        w.act = prev.act;
        w.aux0 = p<void>(prev.Y.rm); w.ldx = prev.Y.ld;
        w.out0 = p<void>(prev.dY.rm); w.ld0 = prev.dY.ld;
        return w;
    }
    // the one-output-channel stage as direct kernels: `prev` produced its input
    ThinSeg thin_seg(const ConvStage& st, const ConvStage& prev) {
        ThinSeg t;
        std::memset(&t, 0, sizeof(t));
        t.g = st.g; t.g.B = B;
        t.X = p<void>(prev.Y.rm);
        t.Wt = p<void>(st.d.Wt);
        t.Y = p<void>(st.Y.rm); t.ldy = st.Y.ld;
        t.act = st.act; t.act_in = prev.act;
        t.dY = p<void>(st.dY.rm); t.lddy = st.dY.ld;
        if (st.dense_map) { t.img_y = st.Y.ld; t.ldy = 1; t.img_dy = st.dY.ld; t.lddy = 1; }      // dense rows: pixel stride 1, image stride = row stride
        t.split = thin_split(h->sw, st.g, 0); t.fast = thin_fast(h->sw, st.g) ? 1 : 0;      // (the training launches set the split of their mode: thin_launch)
        t.dX = p<void>(prev.dY.rm); t.lddx = prev.dY.ld;
        t.part = p<float>(st.thin_part); t.Kp = st.thin_kp;
        return t;
    }
    // tile shape of the element-wise conv helpers: 4*cl columns (cl lanes of a quad each, a power of two <= 16) x (256/cl)*rpt
    // rows; outputs with few columns get tall tiles instead of idle lanes, outputs with few rows one row per thread so
    // that there are enough workgroups
    static void tile_shape(int rows, int cols, int* cl, int* rpt, int* tiles_r, int* tiles_c) {
        int c = 1;
        while (c < 16 && 4 * c < cols) c *= 2;
        *cl = c;
        *rpt = (long)rows * ((cols + 4 * c - 1) / (4 * c)) >= 4L * (kThreads / c) * 512 ? 4 : 1;      // >= 512 workgroups at 4 rows/thread
        const int tr = (kThreads / c) * *rpt;
        *tiles_r = (rows + tr - 1) / tr; *tiles_c = (cols + 4 * c - 1) / (4 * c);
    }
    GatherSeg gather_seg(const ConvStage& st, const void* src) {
        GatherSeg g;
        std::memset(&g, 0, sizeof(g));
        g.g = st.g; g.g.B = B;
        g.src = src;
        g.P = p<void>(st.P.rm); g.ldp = st.P.ld;
        const int M = conv_rows(st), KC = st.d.in + (st.bias ? 1 : 0);
        tile_shape(M, KC, &g.cl, &g.rpt, &g.tiles_r, &g.tiles_c);
        return g;
    }
    // gradient of stage `st`'s input: into the producing stage `prev` (nullptr: latent mode -> dH of `md`)
    Col2imSeg col2im_seg(const ConvStage& st, const ConvStage* prev, const Mod& md) {
        Col2imSeg c;
        std::memset(&c, 0, sizeof(c));
        c.g = st.g; c.g.B = B;
        c.dP = p<float>(st.dP); c.lddp = st.lddp;
        int C;
        if (prev) {
            c.yprev = prev->act == AVAE_ACT_IDENTITY ? nullptr : p<void>(prev->Y.rm); c.ldy = prev->Y.ld; c.act = prev->act;
            c.dA = p<void>(prev->dY.rm); c.lda = prev->dY.ld;
            C = st.g.Cin;
        } else {
            c.g0 = p<float>(md.g0); c.nz = h->nz;
            c.dA = p<void>(md.dH.rm); c.lda = md.dH.ld;
            C = 2 * h->nz;
        }
        const int R = B * st.g.IH * st.g.IW;
        tile_shape(R, C, &c.cl, &c.rpt, &c.tiles_r, &c.tiles_c);
        return c;
    }
    // ---- implicit-GEMM routes (ConvA): descriptors are appended to the handle's table, items carry the 1-based index
    static unsigned magic(int x) { return x <= 1 ? 0u : (unsigned)(0x100000000ull / (unsigned)x) + 1u; }
    int add_conv(const ConvGeom& g, const void* src, bool ones) {
        ConvA c;
        std::memset(&c, 0, sizeof(c));
        c.src = src; c.consts = p<void>(h->off_consts);
        c.M = g.B * g.OH * g.OW; c.K = g.k * g.k * g.Cin;
        c.OHW = g.OH * g.OW; c.OW = g.OW; c.IH = g.IH; c.IW = g.IW; c.Cin = g.Cin;
        c.k = g.k; c.so = g.so; c.d = g.d; c.pad = g.pad; c.src_sb = g.src_sb; c.src_sp = g.src_sp; c.ones = ones ? 1 : 0;
        c.mg_ohw = magic(c.OHW); c.mg_ow = magic(c.OW); c.mg_k = magic(c.k); c.mg_cin = magic(c.Cin);
        if ((c.d != 1 && c.d != 2) || (c.so != 1 && c.so != 2)) throw Err("internal error: implicit conv geometry (strides 1 and 2 only)");
        if ((size_t)h->conv_tab.size() >= 4 * (size_t)kMaxConvA * kMaxMod) throw Err("internal error: too many implicit patch matrices");
        h->conv_tab.push_back(c);
        return (int)h->conv_tab.size();
    }
    // forward of stage `st` on the map `src` (strides in st.g): Y = act(P . W_aug), P implicit
    WorkItem conv_fwd_impl(const ConvStage& st, const void* src) {
        ConvGeom g = st.g; g.B = B;
        WorkItem w = gemm_item(K_FWD_HIDDEN, conv_rows(st), st.d.out, K_of(st.d.in + 1), p<void>(h->off_consts), 0, p<void>(st.d.Wt), st.d.ldt);
        w.act = st.act;
        w.out0 = p<void>(st.Y.rm); w.ld0 = st.Y.ld;
        w.conv = add_conv(g, src, st.bias);
        return w;
    }
    // adjoint geometry of stage `st`: rows = its input pixels, source = its output gradient `dY` (element strides sb / sp)
    ConvGeom adj_geom(const ConvStage& st, int sb, int sp) const {
        const ConvGeom& f = st.g;
        return ConvGeom{B, f.OH, f.OW, st.d.out, f.IH, f.IW, f.k, f.d, f.so, f.k - 1 - f.pad, sb, sp, 0};
    }
    // input gradient of stage `st` as an implicit GEMM on its output gradient: dX = (Padj . Wadj^T) * act'(stored input)
    WorkItem adj_dgrad_impl(const ConvStage& st, const void* dY, int sb, int sp, int prev_act, const Act& prevY, const Act& prevdY) {
        const int rows = B * st.g.IH * st.g.IW, KA = st.g.k * st.g.k * st.d.out;
        WorkItem w = gemm_item(K_DGRAD_HIDDEN, rows, st.g.Cin, K_of(KA), p<void>(h->off_consts), 0, p<void>(st.Wadj), st.ldadj);
        w.act = prev_act;
        w.aux0 = p<void>(prevY.rm); w.ldx = prevY.ld;
        w.out0 = p<void>(prevdY.rm); w.ld0 = prevdY.ld;
        w.conv = add_conv(adj_geom(st, sb, sp), dY, false);
        return w;
    }
    // the first decoder stage's input is z: its input gradient takes the latent epilogue (dz -> [dmu | dlv], reparameterisation)
    WorkItem adj_dgrad_latent_impl(const ConvStage& st, const Mod& md) {
        const int KA = st.g.k * st.g.k * st.d.out;
        WorkItem w = gemm_item(K_DGRAD_LATENT, B, h->nz, K_of(KA), p<void>(h->off_consts), 0, p<void>(st.Wadj), st.ldadj);
        w.nz = h->nz;
        w.aux2 = p<void>(md.g0);
        w.out0 = p<void>(md.dH.rm); w.ld0 = md.dH.ld;
        w.conv = add_conv(adj_geom(st, st.g.OH * st.g.OW * st.dY.ld, st.dY.ld), p<void>(st.dY.rm), false);
        return w;
    }
    // filter gradient of stage `st`: dW_aug = P^T . dA with P implicit (K-major operand of the weight-gradient kernel)
    WorkItem wgrad_impl(const ConvStage& st, const void* src, const Act& dA) {
        ConvGeom g = st.g; g.B = B;
        const int rows = conv_rows(st);
        WorkItem w = gemm_item(K_WGRAD, st.d.in + 1, st.d.out, K_of(rows), p<void>(h->off_consts), 0, p<void>(dA.rm), dA.ld);
        w.out0 = h->grad() + st.d.master; w.ld0 = st.d.ld;
        if (st.ksplit > 1) { w.ksplit = st.ksplit; w.kchunk = st.kchunk; w.out1 = p<void>(st.part); }
        w.conv = add_conv(g, src, st.bias);
        return w;
    }
    // dW_aug[m][n] = sum_k X_aug[k][m] * dA[k][n]: both operands are read as stored (row = sample k), see the K-major
    // ("TN") images in avae_kernels.hip; rows >= batch of either buffer are zero padding
    WorkItem wgrad(const Act& x, const Dense& d, const Act& dA) {
        WorkItem w = gemm_item(K_WGRAD, d.in + 1, d.out, K_of(x.rows), p<void>(x.rm), x.ld, p<void>(dA.rm), dA.ld);
        w.out0 = h->grad() + d.master; w.ld0 = d.ld;
        return w;
    }
    WorkItem wgrad_stage(const ConvStage& st, const Act& dA) {
        WorkItem w = wgrad(st.P, st.d, dA);
        if (st.ksplit > 1) { w.ksplit = st.ksplit; w.kchunk = st.kchunk; w.out1 = p<void>(st.part); }
        return w;
    }
    WorkItem latent() {
        WorkItem w;
        std::memset(&w, 0, sizeof(w));
        w.kind = K_LATENT; w.M = B; w.nz = h->nz; w.n_mod = h->M;
        const float bg = (float)(h->cfg.batch_global > 0 ? h->cfg.batch_global : h->cfg.batch_size);
        w.inv_bg = 1.0f / bg; w.lambda = h->cfg.assoc_lambda;
        const void** in_slots[kMaxMod] = {&w.A, &w.B, &w.aux0, &w.aux1};
        void** out_slots[kMaxMod - 1] = {&w.out0, &w.out1, &w.out2};
        for (int m = 0; m < h->M; ++m) {
            *in_slots[m] = p<void>(h->mods[m].mulv);
            if (m < kMaxMod - 1) *out_slots[m] = p<void>(h->mods[m].g0); else w.aux2 = p<void>(h->mods[m].g0);
            w.wts[m] = h->cfg.mod[m].weight;
        }
        w.eps = p<float>(h->off_eps); w.ldx = h->ld_eps;
        w.partial = p<float>(h->off_partial);
        return w;
    }
    WorkItem cost(bool bump) {
        WorkItem w;
        std::memset(&w, 0, sizeof(w));
        w.kind = K_COST; w.partial = p<float>(h->off_partial); w.bump_step = bump ? 1 : 0;
        w.scale = h->cfg.learning_rate; w.lambda = h->cfg.beta1; w.inv_bg = h->cfg.beta2;
        w.out0 = h->grad() + h->P_int;
        return w;
    }
};

inline bool is_gemm(int kind) { return kind <= K_WGRAD || kind == K_DGRAD_F32 || kind == K_SERVE_Z; }

// finish_launch, step 1: the tile configuration of a launch of items [first, first + count) -- a function of the items and the switches.
TileCfg choose_cfg(const std::vector<WorkItem>& items, int first, int count, const PlanSwitches& sw) {
    bool need128 = false, narrow = false;
    long tiles128 = 0;
    for (int i = first; i < first + count; ++i) {
        const WorkItem& w = items[i];
        if ((w.kind == K_FWD_HEAD || w.kind == K_DGRAD_LATENT) && 2 * w.nz > 64) need128 = true;
        if (is_gemm(w.kind)) tiles128 += (long)((w.M + 127) / 128) * ((w.N + 127) / 128);
        if (is_gemm(w.kind) && (w.N <= 64 || w.M <= 64 || w.conv > 0)) narrow = true;      // a 128-wide tile would be mostly padding (implicit patch matrices: small tiles only)
    }
    TileCfg cfg = (need128 || (tiles128 >= 192 && !narrow)) ? k128x128 : k64x64;
    {   // 256x128 tiles, 8 waves, one workgroup per CU: a third more flops per operand byte pulled from L2 into LDS,
        // and that fill rate (~60-70 GB/s per CU) is what bounds the 128x128 loop.  Plain single-C-tile kinds on big
        // problems only.  (AVAE_NO_256=1 keeps the 128x128 kernel: A/B measurements.)
        bool plain = !sw.no_256;
        long tiles256 = 0;
        for (int i = first; i < first + count; ++i) {
            const WorkItem& w = items[i];
            plain = plain && (w.kind == K_FWD_HIDDEN || w.kind == K_DGRAD_HIDDEN || w.kind == K_WGRAD);
            tiles256 += (long)((w.M + 255) / 256) * ((w.N + 127) / 128);
        }
        if (cfg == k128x128 && plain && tiles256 >= 192) cfg = k256x128;
    }
    if (cfg == k64x64 && !sw.no_32) {      // few 64x64 tiles: half-height tiles put twice the CUs on the launch
        long t64 = 0;
        bool nt = true;
        for (int i = first; i < first + count; ++i) {
            const WorkItem& w = items[i];
            if (is_gemm(w.kind)) t64 += (long)((w.M + 63) / 64) * ((w.N + 63) / 64);
            nt = nt && w.kind != K_WGRAD && w.kind != K_DGRAD_F32;
        }
        if (nt && t64 > 0 && t64 <= 128) cfg = k32x64;
        bool head = false;
        for (int i = first; i < first + count; ++i) head = head || items[i].kind == K_FWD_HEAD || items[i].kind == K_DGRAD_LATENT || items[i].kind == K_SERVE_Z;
        if (cfg == k32x64 && !head && !sw.no_32x32) cfg = k32x32;      // no kind that needs 2*n_z columns in one tile
        if (cfg == k32x32 && !sw.no_lean) {       // the chain's two kinds, one of them (and one transfer function) per launch: the lean kernel (k_small)
            bool lean = true;
            const int k0 = items[first].kind, a0 = items[first].act;
            for (int i = first; i < first + count; ++i)
                lean = lean && items[i].kind == k0 && items[i].act == a0 && !items[i].bias_ep && items[i].K > 0 && items[i].conv == 0;
            if (lean && (k0 == K_FWD_HIDDEN || k0 == K_DGRAD_HIDDEN)) cfg = kLean;
            bool store = true;                                    // the inference / serving output launch: k_small's third kind
            for (int i = first; i < first + count; ++i) store = store && items[i].kind == K_FWD_OUT_STORE && !items[i].bias_ep && items[i].K > 0 && items[i].conv == 0;
            if (store) cfg = kLean;
            bool loss = false, only_loss = true;                  // the output + loss launch (with the latent item riding in it): k_small_loss
            for (int i = first; i < first + count; ++i) {
                loss = loss || items[i].kind == K_FWD_OUT_LOSS;
                only_loss = only_loss && ((items[i].kind == K_FWD_OUT_LOSS && !items[i].bias_ep && items[i].K > 0 && items[i].conv == 0) || items[i].kind == K_LATENT);
            }
            if (cfg == k32x32 && loss && only_loss && !sw.no_lean_loss) cfg = kLeanLoss;
        }
    }
    if (cfg == k128x128 && need128 && !sw.no_64x128) {      // wide-latent head launches: few tiles, K loop = load latency
        long t = 0;
        bool nt = true;
        for (int i = first; i < first + count; ++i) {
            const WorkItem& w = items[i];
            if (is_gemm(w.kind)) t += (long)((w.M + 63) / 64) * ((w.N + 127) / 128);
            nt = nt && w.kind != K_WGRAD && w.kind != K_DGRAD_F32;
        }
        if (nt && t <= 256) cfg = k64x128;
    }
    if (cfg == k128x128 && !sw.no_loss8) {      // the output + loss launch of the big nets: 256x64 tiles, 8 waves, register epilogue
        long t = 0;
        bool loss_only = true;
        for (int i = first; i < first + count; ++i) {
            const WorkItem& w = items[i];
            if (is_gemm(w.kind)) { loss_only = loss_only && w.kind == K_FWD_OUT_LOSS; t += (long)((w.M + 255) / 256) * ((w.N + 63) / 64); }
        }
        if (loss_only && t >= 192) cfg = k256x64Loss;
    }
    for (int i = first; i < first + count; ++i)
        if (items[i].conv > 0 && !tile_geom(cfg).gather) throw Err("internal error: an implicit patch matrix on a tile configuration without the gather");
    return cfg;
}

// step 2 (8-wave NT tiles): the bias moves into the epilogue where that saves a K tile
void fold_bias_epilogue(std::vector<WorkItem>& items, int first, int count, int KU) {
    for (int i = first; i < first + count; ++i) {
        WorkItem& w = items[i];
        if ((w.kind == K_FWD_HIDDEN || w.kind == K_FWD_OUT_LOSS) && w.kin > 0 && w.kin % KU == 0 && w.K == w.kin + KU) { w.K = w.kin; w.bias_ep = 1; }
    }
}

// step 3: the items' tiles on the configuration's tile shape and their cost-partial slots; returns the longest item's tile count
int layout_tiles(std::vector<WorkItem>& items, int first, int count, TileCfg cfg, const PlanSwitches& sw, int* next_slot) {
    const int T = tile_geom(cfg).cols, TM = tile_geom(cfg).rows;
    int max_tiles = 1;
    for (int i = first; i < first + count; ++i) {
        WorkItem& w = items[i];
        if (is_gemm(w.kind)) {
            if (w.bias_row >= 0) {       // (< 0: a product without a bias row, e.g. the adjoint-frame filter gradients)
                w.bias_row = 0;
                if (w.kind == K_WGRAD && w.M > 1 && (w.M - 1) % TM == 0 && !sw.no_bias_mfma) w.bias_row = w.M - 1;
            }
            w.tiles_m = (w.M - (w.bias_row > 0 ? 1 : 0) + TM - 1) / TM;
            w.tiles_n = (w.N + T - 1) / T;
            if ((w.kind == K_FWD_HEAD || w.kind == K_DGRAD_LATENT) && w.tiles_n != 1) throw Err("internal error: head tile");
            if (w.kind == K_FWD_OUT_LOSS) { w.slot_base = *next_slot; *next_slot += w.tiles_m * w.tiles_n; }
        } else if (w.kind == K_LATENT) {
            w.tiles_m = (w.M + kLatentRows - 1) / kLatentRows; w.tiles_n = 1;
            w.slot_base = *next_slot; *next_slot += w.tiles_m;
        } else {   // K_COST
            w.tiles_m = w.tiles_n = 1;
            w.n_slots = *next_slot;
        }
        max_tiles = std::max(max_tiles, w.tiles_m * w.tiles_n * (w.kind == K_WGRAD && w.ksplit > 1 ? w.ksplit : 1));
    }
    return max_tiles;
}

// step 4 (weight-gradient launches): the entry table of L.targs.  The grid is (longest entry) x (entries), so layers of very
// different size would make it mostly padding workgroups (C2: 1248 workgroups for 416 tiles).  Items are therefore cut into
// entries of at most SX tiles, SX chosen to launch the fewest workgroups within the entry table's size.  Returns the entry
// count; *G = the XCD group, *SX = the slice width.
int wgrad_entries(Launch& L, const std::vector<WorkItem>& items, const PlanSwitches& sw, int* G_out, int* SX_out) {
    const int first = L.first, count = L.count;
    // big weight gradients: concentrate each item on 8/G XCDs (the launch is bound by L2 misses); G must leave no XCD
    // without an item, so it divides the item count
    int G = 1;
    if (L.cfg == k256x128) for (int g : {4, 2}) if (count % g == 0) { G = g; break; }
    if (sw.tn_g_set) G = sw.tn_g;
    if (G != 1 && G != 2 && G != 4 && G != 8) throw Err("AVAE_TN_G must be 1, 2, 4 or 8");
    auto tiles_of = [&](const WorkItem& w) { return w.tiles_m * w.tiles_n * (w.ksplit > 1 ? w.ksplit : 1); };
    int SX = L.grid_x;
    if (G == 1 && !sw.no_tn_slices) {
        long best = -1;
        for (int sx = 8; sx <= L.grid_x; sx += 8) {
            long entries = 0;
            for (int i = first; i < first + count; ++i) entries += (tiles_of(items[i]) + sx - 1) / sx;
            if (entries > kMaxTnItems) continue;
            if (best < 0 || entries * sx <= best) { best = entries * sx; SX = sx; }
        }
    }
    int n = 0;
    for (int i = 0; i < count; ++i) {
        const WorkItem& w = items[first + i];
        const int nt = tiles_of(w);
        for (int off = 0; off < nt; off += SX) {
            if (n >= kMaxTnItems) throw Err("internal error: too many weight-gradient entries");
            TnItem& t = L.targs.items[n++];
            t.A = w.A; t.B = w.B; t.out = reinterpret_cast<float*>(w.ksplit > 1 ? w.out1 : w.out0);
            t.bias_row = std::max(w.bias_row, 0);
            t.M = w.bias_row > 0 ? w.M - 1 : w.M; t.N = w.N; t.K = w.K; t.lda = w.lda; t.ldb = w.ldb; t.ld0 = w.ld0;
            t.tiles_m = w.tiles_m; t.tiles_n = w.tiles_n; t.ksplit = w.ksplit; t.kchunk = w.kchunk;
            t.tile_off = off; t.tile_cnt = std::min(SX, nt - off); t.conv = w.conv;
        }
    }
    *G_out = G; *SX_out = SX;
    return n;
}

// step 5 (G > 1): entries over the XCD groups.  Returns the new entry count; *G may drop from 4 to 2.
int balance_xcd_groups(Launch& L, int n, const PlanSwitches& sw, int* G_io) {
    int G = *G_io;
    // Entry y of a group of G runs on XCDs [ (y % G) * 8/G, ... ): its position decides WHERE its tiles run.  Layers
    // differ in size (C4: 32, 28, 8 and 4 tiles), and in plan order two of the four XCD pairs end up with 66 tiles per
    // XCD -- a third round of 62 us for four tiles on a 32-CU XCD (195 us; the other XCDs are done after 138).  Longest
    // first onto the lightest position balances the positions; G = 4 or 2 by the fewest rounds that leaves.
    std::vector<TnItem> ent(L.targs.items, L.targs.items + n);
    std::stable_sort(ent.begin(), ent.end(), [](const TnItem& a, const TnItem& b) { return a.tile_cnt > b.tile_cnt; });
    auto pack = [&](int g, std::vector<std::vector<TnItem>>& bins) {
        bins.assign(g, {});
        std::vector<long> load(g, 0);
        const int cap = kMaxTnItems / g;
        for (const TnItem& e : ent) {
            int best = -1;
            for (int p = 0; p < g; ++p) if ((int)bins[p].size() < cap && (best < 0 || load[p] < load[best])) best = p;
            bins[best].push_back(e); load[best] += e.tile_cnt;
        }
        const long per_xcd = (*std::max_element(load.begin(), load.end()) * g + 7) / 8;
        return (per_xcd + 31) / 32;                       // rounds on a 32-CU XCD at one workgroup per CU
    };
    std::vector<std::vector<TnItem>> bins, bins2;
    if (!sw.tn_g_set && G == 4 && n * 2 <= kMaxTnItems * 2) {
        const long r4 = pack(4, bins), r2 = pack(2, bins2);
        if (r2 < r4) { G = 2; bins.swap(bins2); }
    } else {
        pack(G, bins);
    }
    size_t groups = 0;
    for (const auto& bn : bins) groups = std::max(groups, bn.size());
    std::memset(L.targs.items, 0, sizeof(L.targs.items));
    for (size_t g = 0; g < groups; ++g)
        for (int p = 0; p < G; ++p) if (g < bins[p].size()) L.targs.items[g * G + p] = bins[p][g];      // holes: tile_cnt 0
    n = (int)groups * G;
    *G_io = G;
    return n;
}

// Fixes the tile configuration of one launch and lays its items' tiles out back to back.
Launch finish_launch(avae_handle* h, std::vector<WorkItem>& items, int first, int count, const std::string& name, int* next_slot) {
    const PlanSwitches& sw = h->sw;
    Launch L;
    L.name = name; L.first = first; L.count = count;
    L.cfg = choose_cfg(items, first, count, sw);
    if (tile_geom(L.cfg).waves8 && !sw.no_bias_ep) fold_bias_epilogue(items, first, count, h->KU);
    const int max_tiles = layout_tiles(items, first, count, L.cfg, sw, next_slot);
    // grid: x = tile slot (multiple of 8: the kernel's XCD-aware tile order needs it), y = item
    L.grid_x = (max_tiles + 7) & ~7; L.grid_y = count;
    L.blocks = L.grid_x * L.grid_y;
    bool two = false;
    for (int i = first; i < first + count; ++i) two = two || items[i].kind == K_FWD_HEAD || items[i].kind == K_DGRAD_LATENT || items[i].kind == K_SERVE_Z;
    L.lds = L.cfg == kLean ? tile_ring_bytes(kLean) : L.cfg == kLeanLoss ? tile_ring_bytes(kLeanLoss) + 64 : tile_lds_bytes(L.cfg, two);
    L.tn = true;
    for (int i = first; i < first + count; ++i) L.tn = L.tn && items[i].kind == K_WGRAD;
    if (count > (L.tn ? kMaxTnItems : kMaxItemsPerLaunch)) throw Err("internal error: too many items in one launch");
    std::memset(&L.args, 0, sizeof(L.args));
    std::memset(&L.targs, 0, sizeof(L.targs));
    if (L.tn) {
        int G = 1, SX = L.grid_x;
        int n = wgrad_entries(L, items, sw, &G, &SX);
        if (G > 1 && !sw.no_tn_balance) n = balance_xcd_groups(L, n, sw, &G);
        L.grid_x = SX;
        L.targs.n_items = n;
        L.targs.grid_x = L.grid_x;
        L.targs.xcd_group = G;
        L.grid_y = (n + G - 1) / G * G;
        L.blocks = L.grid_x * L.grid_y;
    } else {
        L.args.n_items = count;
        L.args.grid_x = L.grid_x;
        for (int i = 0; i < count; ++i) L.args.items[i] = items[first + i];
    }
    L.args.conv_tab = L.targs.conv_tab = h->at<ConvA>(h->off_conv_tab);
    L.args.sched = L.targs.sched = sw.sched;
    if (*next_slot > h->n_partial) throw Err("internal error: cost partial slots overflow");
    return L;
}

void dp_ranges(const avae_handle* h, int* n_buckets, std::vector<avae_handle::Range> (&out)[2]);

// k_small_tn: hand every XCD its own list of (layer, tile range) -- TnLaunchArgs::pieces.  The launch's entries (layers cut into
// slices for the grid's sake) are merged back into whole layers; the layers, longest first, go whole to the fullest XCD that still
// has room under the quota of ceil(tiles / 8) (best fit), and a layer that fits nowhere is cut: the emptiest XCD is filled up and
// the rest tried again.  Leaves the launch as it was when an XCD would need more than kTnPieces pieces.
void xcd_pieces(Launch& L) {
    TnLaunchArgs& a = L.targs;
    std::vector<TnItem> layers;
    for (int i = 0; i < a.n_items; ++i) {
        const TnItem& e = a.items[i];
        if (e.tile_cnt <= 0) continue;
        bool seen = false;
        for (const TnItem& l : layers) seen = seen || l.out == e.out;
        if (seen) continue;
        TnItem l = e;
        l.tile_off = 0; l.tile_cnt = e.tiles_m * e.tiles_n;
        if (l.tile_cnt > 65535) return;
        layers.push_back(l);
    }
    long total = 0;
    for (const TnItem& l : layers) total += l.tile_cnt;
    if (layers.empty() || total > 8L * 65535) return;
    const int quota = (int)((total + 7) / 8);
    std::vector<int> order(layers.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return layers[x].tile_cnt > layers[y].tile_cnt; });
    struct Bin { int load = 0; std::vector<TnPiece> pc; };
    Bin bins[8];
    for (int li : order) {
        int off = 0, left = layers[li].tile_cnt;
        while (left > 0) {
            int best = -1;
            for (int b = 0; b < 8; ++b)          // whole (what is left of it): the fullest XCD it fits
                if ((int)bins[b].pc.size() < kTnPieces && bins[b].load + left <= quota && (best < 0 || bins[b].load > bins[best].load)) best = b;
            int take = left;
            if (best < 0) {                      // cut: fill the emptiest XCD
                for (int b = 0; b < 8; ++b)
                    if ((int)bins[b].pc.size() < kTnPieces && bins[b].load < quota && (best < 0 || bins[b].load < bins[best].load)) best = b;
                if (best < 0) return;
                take = std::min(left, quota - bins[best].load);
            }
            bins[best].load += take;
            bins[best].pc.push_back(TnPiece{(unsigned short)li, (unsigned short)off, (unsigned short)bins[best].load, 0});
            off += take; left -= take;
        }
    }
    int longest = 0;
    for (int b = 0; b < 8; ++b) {
        longest = std::max(longest, bins[b].load);
        for (int i = 0; i < kTnPieces; ++i)
            a.pieces[b][i] = i < (int)bins[b].pc.size() ? bins[b].pc[i] : TnPiece{0, 0, (unsigned short)bins[b].load, 0};
    }
    std::memset(a.items, 0, sizeof(a.items));
    for (size_t i = 0; i < layers.size(); ++i) a.items[i] = layers[i];
    a.n_items = (int)layers.size();
    a.xcd_pieces = 1;
    L.grid_x = 8 * longest; L.grid_y = 1; L.blocks = L.grid_x;
    a.grid_x = L.grid_x;
}

// Launch groups of the training, serve and completion plans: group(name, dst, fill) turns the work items that fill() pushes onto
// the plan's table into one launch of dst (none when it pushed nothing).
struct Groups {
    avae_handle* h;
    std::vector<WorkItem>& items;
    int slot = 0;                          // finish_launch's running slot
    template <typename Fill> void operator()(const std::string& name, std::vector<Launch>& dst, Fill&& fill) {
        const int first = (int)items.size();
        fill();
        const int count = (int)items.size() - first;
        if (count > 0) dst.push_back(finish_launch(h, items, first, count, name, &slot));
    }
};

// Small nets: the launch that follows the heads (the decoder's first layer, K = n_z + 1) and the one that follows bwd_dec1_latent
// (the heads' input gradient, K = 2 n_z) multiply over one or two K tiles and are pure launch overhead (4.3 us each on C2).  When the
// producing launch runs on 32x64 tiles they become the tail product of its items (WorkItem::tail_*) and disappear.  The weights
// they read are final since the previous step's Adam, their inputs exist only in the producing workgroup -- nothing else changes.
bool fuse_tail(avae_handle* h, std::vector<Launch>& ls, int mode) {
    if (ls.size() < 2 || h->sw.no_tail) return false;
    Launch& Lp = ls[ls.size() - 2];          // producer: fwd_head / bwd_dec1_latent
    Launch& Lc = ls[ls.size() - 1];          // consumer: one K tile
    if (Lp.type != kGrouped || Lc.type != kGrouped || Lp.tn || Lc.tn || Lp.cfg != k32x64) return false;
    const int want_p = mode == 1 ? K_FWD_HEAD : K_DGRAD_LATENT, want_c = mode == 1 ? K_FWD_HIDDEN : K_DGRAD_HIDDEN;
    std::vector<int> prod(Lc.count, -1);
    for (int i = 0; i < Lc.count; ++i) {
        const WorkItem& c = h->items[Lc.first + i];
        if (c.kind != want_c || c.bias_ep || c.K > 2 * h->KU || c.N > 1024) return false;      // (the narrow result is one 64-column tile)
        for (int k = 0; k < Lp.count; ++k) {
            const WorkItem& n = h->items[Lp.first + k];
            if (n.kind != want_p || n.M != c.M) continue;
            const void* res = mode == 1 ? n.out1 : n.out0;
            const int ldres = mode == 1 ? n.ld1 : n.ld0;
            if (res && res == c.A && ldres == c.lda) prod[i] = k;
        }
        if (prod[i] < 0) return false;
    }
    for (int i = 0; i < Lc.count; ++i) {
        const WorkItem c = h->items[Lc.first + i];
        for (WorkItem* n : {&h->items[Lp.first + prod[i]], &Lp.args.items[prod[i]]}) {
            n->tail_mode = mode; n->tail_w = c.B; n->tail_ldw = c.ldb; n->tail_n = c.N; n->tail_out = c.out0; n->tail_ldo = c.ld0;
            n->tail_aux = c.aux0; n->tail_ldx = c.ldx; n->tail_act = c.act; n->tail_kt = c.K / h->KU;
            n->tiles_n = (c.N + 63) / 64;                    // tail slices of 64 columns, a workgroup each
        }
    }
    int max_tiles = 1;
    for (int k = 0; k < Lp.count; ++k) max_tiles = std::max(max_tiles, h->items[Lp.first + k].tiles_m * h->items[Lp.first + k].tiles_n);
    Lp.grid_x = (max_tiles + 7) & ~7; Lp.blocks = Lp.grid_x * Lp.grid_y; Lp.args.grid_x = Lp.grid_x;
    Lp.name += "+" + Lc.name;
    ls.pop_back();
    // the lean frame for the fused head launches (k_small_latb): every GEMM item of the kind, one transfer function, its narrow result and
    // the consumer's K within the 8-KiB image
    if (!h->sw.no_lean && !h->sw.no_lean_head) {
        bool lean = true;
        int act = -1;
        for (int k = 0; k < Lp.count; ++k) {
            const WorkItem& n = h->items[Lp.first + k];
            if (n.kind == K_COST) continue;
            lean = lean && n.kind == want_p && n.tail_mode == mode
                        && (act < 0 || act == n.tail_act) && n.K > 0 && 2 * n.nz <= 64 && n.tail_kt >= 1 && n.tail_kt <= 2;
            act = n.tail_act;
        }
        if (lean && mode == 1)
            for (int k = 0; k < Lp.count; ++k) lean = lean && h->items[Lp.first + k].kind == K_FWD_HEAD && h->items[Lp.first + k].out1 != nullptr;
        if (lean) { Lp.cfg = mode == 2 ? kLeanLatb : kLeanHead; Lp.lds = small_head_lds_bytes(); Lp.lean_act = act; }
    }
    return true;
}

// conv-branch helper launches (one segment per conv modality)
// (`want`: which conv modalities take part -- stages route per modality: patch-matrix, adjoint-frame or direct)
template <typename StageOf, typename SrcOf, typename Want>
void gather_launch(avae_handle* h, Builder& bd, const std::string& name, std::vector<Launch>& dst, StageOf&& stage_of, SrcOf&& src_of, Want&& want) {
    Launch L;
    L.name = name; L.type = kGather;
    int base = 0;
    for (Mod& md : h->mods) if (md.conv && want(md)) {
        GatherSeg g = bd.gather_seg(stage_of(md), src_of(md));
        g.tile_base = base; base += g.tiles_r * g.tiles_c;
        L.ga.seg[L.ga.n_seg++] = g;
    }
    L.blocks = base;
    if (base > 0) dst.push_back(L);
}
template <typename StageOf, typename PrevOf, typename Want>
void col2im_launch(avae_handle* h, Builder& bd, const std::string& name, std::vector<Launch>& dst, StageOf&& stage_of, PrevOf&& prev_of, Want&& want) {
    Launch L;
    L.name = name; L.type = kCol2im;
    int base = 0;
    for (Mod& md : h->mods) if (md.conv && want(md)) {
        Col2imSeg c = bd.col2im_seg(stage_of(md), prev_of(md), md);
        c.tile_base = base; base += c.tiles_r * c.tiles_c;
        L.ca.seg[L.ca.n_seg++] = c;
    }
    L.blocks = base;
    if (base > 0) dst.push_back(L);
}
// the decoder's last transposed conv (one output channel) runs as direct kernels: mode 0 forward, 1 input gradient,
// 2 filter-gradient partial sums
void thin_launch(avae_handle* h, Builder& bd, const std::string& name, std::vector<Launch>& dst, int mode, int i) {
    Launch L;
    L.name = name; L.type = kThin;
    L.ta.mode = mode;
    int base = 0;
    for (Mod& md : h->mods) if (md.conv && md.cdec[i].thin) {
        ThinSeg t = bd.thin_seg(md.cdec[i], md.cdec[i - 1]);
        t.split = thin_split(h->sw, md.cdec[i].g, mode);
        t.block_base = base;
        base += h->B * t.split;                        // workgroups per image
        L.ta.seg[L.ta.n_seg++] = t;
    }
    L.blocks = base;
    if (base > 0) dst.push_back(L);
}

// Experiment (AVAE_CHAIN2=1): fwd_enc1 and fwd_enc2 of the small nets as ONE launch behind a row-block-local hand-off
// (k_chain2) instead of a kernel boundary.  Needs both on the lean 32x32 kernel, equal widths (the same tile grid) and whole quads.
void chain_enc12(avae_handle* h) {
    if (h->plain.fwd.size() == 2 && h->plain.fwd[0].cfg == kLean && h->plain.fwd[1].cfg == kLean && h->plain.fwd[0].count == h->plain.fwd[1].count
        && 2 * h->plain.fwd[0].count <= kMaxItemsPerLaunch) {
        Launch& A = h->plain.fwd[0];
        const Launch& Bn = h->plain.fwd[1];
        bool ok = true;
        for (int i = 0; i < A.count; ++i) {
            const WorkItem& a = A.args.items[i];
            const WorkItem& c = Bn.args.items[i];
            ok = ok && a.kind == K_FWD_HIDDEN && c.kind == K_FWD_HIDDEN && a.act == c.act && a.M == c.M && a.N == c.N && a.tiles_m == c.tiles_m && a.tiles_n == c.tiles_n
                    && c.A == a.out0 && c.lda == a.ld0 && a.N % 4 == 0 && a.tiles_m <= 64;
        }
        if (ok) {
            for (int i = 0; i < A.count; ++i) A.args.items[A.count + i] = Bn.args.items[i];
            A.args.n_items = 2 * A.count;
            A.cfg = kChain2; A.name += "+" + Bn.name;
            h->plain.fwd.pop_back();
        }
    }
}

// Launches are classified by their names: the conv modality's own launches start with "conv_", and a launch that has taken
// another one in carries a '+'.
inline bool is_conv_launch(const Launch& L) { return L.name.compare(0, 5, "conv_") == 0; }
inline bool is_merged(const Launch& L) { return L.name.find('+') != std::string::npos; }

// ---- mixed models: the MLP modalities' hidden-layer launches (a few tiles, 4-5 us each as launches of their own) ride in plain
// GEMM launches of the conv modality.  Taken from the end of each chain backwards, a launch SINKS into the LATEST such launch
// that still runs before the first reader of its outputs -- so a chain enc1 -> enc2 ends up in two consecutive conv launches.
// Where no such launch lies between a launch and its reader (the backward pass: the MLP modality's dgrad layers come after the
// conv decoder's), it is HOISTED into the earliest one behind the writer of its input gradient.
// Safe: every buffer is written once per step, so a product may run any time between its inputs' writers and its readers.
void sink_and_hoist(avae_handle* h) {
    auto plain_kind = [](int k) { return k == K_FWD_HIDDEN || k == K_DGRAD_HIDDEN || k == K_DGRAD_F32; };
    // only launches of the MLP modalities move: an item that writes a conv modality's buffer stays where the plan put it (its readers
    // include helper launches -- the direct stage, im2col / col2im -- that the dependency scans below do not look into)
    std::vector<const void*> conv_bufs;
    for (const Mod& md : h->mods) if (md.conv) {
        for (const Act* a : {&md.Z, &md.dH, &md.dO}) conv_bufs.push_back(h->at<void>(a->rm));
        for (const std::vector<ConvStage>* side : {&md.cenc, &md.cdec})
            for (const ConvStage& st : *side) { conv_bufs.push_back(h->at<void>(st.Y.rm)); conv_bufs.push_back(h->at<void>(st.dY.rm)); }
    }
    auto mlp_item = [&](const WorkItem& w) {
        if (w.conv > 0) return false;
        for (const void* q : conv_bufs) if (q == w.out0 || q == w.A) return false;
        return true;
    };
    auto reads = [&](const Launch& L, const std::vector<const void*>& outs) {
        if (L.type != kGrouped) return false;           // the conv helper launches touch the conv modality's buffers only
        for (int i = 0; i < L.count; ++i) {
            const WorkItem& w = h->items[L.first + i];
            const void* csrc = w.conv > 0 ? h->conv_tab[w.conv - 1].src : nullptr;      // (an implicit patch matrix reads its source map)
            for (const void* q : {w.A, w.B, w.aux0, w.aux1, w.aux2, (const void*)w.tail_w, (const void*)w.tail_aux, csrc})
                for (const void* o : outs) if (q && q == o) return true;
        }
        return false;
    };
    auto writes = [&](const Launch& L, const std::vector<const void*>& ins) {
        if (L.type != kGrouped) return false;
        for (int i = 0; i < L.count; ++i) {
            const WorkItem& w = h->items[L.first + i];
            for (const void* q : {(const void*)w.out0, (const void*)w.out1, (const void*)w.tail_out})
                for (const void* o : ins) if (q && q == o) return true;
        }
        return false;
    };
    // may launch P move?  An unmerged launch of MLP hidden layers; `ends` gets its items' outputs (outs) or inputs.
    auto movable = [&](const Launch& P, bool outs, std::vector<const void*>& ends) {
        if (P.type != kGrouped || P.tn || is_conv_launch(P) || is_merged(P)) return false;
        for (int i = 0; i < P.count; ++i) {
            const WorkItem& w = h->items[P.first + i];
            if (!((w.kind == K_FWD_HIDDEN || w.kind == K_DGRAD_HIDDEN) && !w.bias_ep && mlp_item(w))) return false;
            ends.push_back(outs ? w.out0 : w.A);
        }
        return true;
    };
    // may launch Q take P in?  A plain GEMM launch of the conv modality off the 8-wave tiles, with room for P's items.
    auto hosts = [&](const Launch& Q, const Launch& P) {
        bool ok = Q.type == kGrouped && !Q.tn && is_conv_launch(Q) && Q.count + P.count <= kMaxItemsPerLaunch && !tile_geom(Q.cfg).waves8;
        for (int i = 0; ok && i < Q.count; ++i) ok = plain_kind(h->items[Q.first + i].kind);
        return ok;
    };
    // ls[a] rides in ls[target]: the items of both, laid out again as one launch; `split` (an index into ls) follows the removal
    auto merge = [&](std::vector<Launch>& ls, int a, int target, int* split) {
        const Launch &P = ls[a], &Q = ls[target];
        const int first = (int)h->items.size();
        for (int i = 0; i < Q.count; ++i) { const WorkItem w = h->items[Q.first + i]; h->items.push_back(w); }
        for (int i = 0; i < P.count; ++i) { const WorkItem w = h->items[P.first + i]; h->items.push_back(w); }
        int dummy_slot = 0;                          // (no kind in here owns cost-partial slots)
        Launch merged = finish_launch(h, h->items, first, Q.count + P.count, Q.name + "+" + P.name, &dummy_slot);
        ls[target] = merged;
        ls.erase(ls.begin() + a);
        if (split && a < *split) --*split;
    };
    auto sink = [&](std::vector<Launch>& ls, int* split) {
        for (int a = (int)ls.size() - 1; a >= 0; --a) {
            std::vector<const void*> outs;
            if (!movable(ls[a], true, outs)) continue;
            int target = -1;
            for (int q = a + 1; q < (int)ls.size() && !reads(ls[q], outs); ++q)
                if (hosts(ls[q], ls[a])) target = q;
            if (target >= 0) merge(ls, a, target, split);
        }
    };
    auto hoist = [&](std::vector<Launch>& ls, int* split) {
        for (int a = 0; a < (int)ls.size(); ++a) {
            std::vector<const void*> ins;
            if (!movable(ls[a], false, ins)) continue;
            int writer = -1;
            for (int q = 0; q < a; ++q) if (writes(ls[q], ins)) writer = q;
            if (writer < 0) continue;                    // (its input comes from the other list: leave it where the plan put it)
            int target = -1;
            for (int q = writer + 1; q < a && target < 0; ++q)
                if (hosts(ls[q], ls[a])) target = q;
            if (target >= 0) { merge(ls, a, target, split); --a; }
        }
    };
    sink(h->plain.fwd, nullptr);
    sink(h->bwd, &h->bwd_split);
    hoist(h->bwd, &h->bwd_split);
}

// does some conv modality route decoder stage i through the adjoint frame / the direct kernels?
bool any_adj(const avae_handle* h, int i) { bool t = false; for (const Mod& md : h->mods) t = t || (md.conv && i >= 0 && i <= 3 && md.cdec[i].adj); return t; }
bool any_thin(const avae_handle* h, int i) { bool t = false; for (const Mod& md : h->mods) t = t || (md.conv && md.cdec[i].thin); return t; }

// Every weight gradient in the last launch(es) of the step: they depend only on stored activations /
// activation gradients, and nothing reads the weights after them, so k_adam follows directly (after the all-reduce
// under data parallelism).  Fusing Adam into these epilogues was measured and dropped: equal on the small nets
// (C2 91.5 vs 91.2 us/step), slower on the big ones (C4 958 vs 922: a fused tile streams 448 KB and stalls the
// MFMA loops it alternates with).
void plan_weight_gradients(avae_handle* h, Builder& bd, Groups& group) {
    std::vector<WorkItem> wg;
    for (Mod& md : h->mods) {
        if (md.conv) {
            if (md.cdec[3].dense_map) wg.push_back(bd.wgrad(md.cdec[3].Y, md.cdec[4].d, md.dO));       // the dense output layer on the dense map
            else wg.push_back(bd.wgrad_stage(md.cdec[4], md.dO));
            for (int i = 3; i >= 0; --i) {
                const ConvStage& st = md.cdec[i];
                if (st.thin) continue;
                if (st.impl_w) wg.push_back(bd.wgrad_impl(st, i == 0 ? h->at<void>(md.Z.rm) : h->at<void>(md.cdec[i - 1].Y.rm), st.dY));
                else if (st.adj) wg.push_back(bd.adj_wgrad(st, md.cdec[i - 1]));
                else wg.push_back(bd.wgrad_stage(st, st.dY));
            }
            if (md.cenc[3].impl_w) wg.push_back(bd.wgrad_impl(md.cenc[3], h->at<void>(md.cenc[2].Y.rm), md.dH));
            else wg.push_back(bd.wgrad_stage(md.cenc[3], md.dH));
            for (int i = 2; i >= 0; --i) {
                const ConvStage& st = md.cenc[i];
                if (st.impl_w) wg.push_back(bd.wgrad_impl(st, i == 0 ? h->at<void>(md.X0.rm) : h->at<void>(md.cenc[i - 1].Y.rm), st.dY));
                else wg.push_back(bd.wgrad_stage(st, st.dY));
            }
            continue;
        }
        wg.push_back(bd.wgrad(md.D.back(), md.outl, md.dO));
        for (int k = md.L - 1; k >= 1; --k) wg.push_back(bd.wgrad(md.D[k - 1], md.dec[k], md.dD[k]));
        wg.push_back(bd.wgrad(md.Z, md.dec[0], md.dD[0]));
        wg.push_back(bd.wgrad(md.E.back(), md.head, md.dH));
        for (int k = md.L - 1; k >= 1; --k) wg.push_back(bd.wgrad(md.E[k - 1], md.enc[k], md.dE[k]));
        wg.push_back(bd.wgrad(md.X0, md.enc[0], md.dE[0]));
    }
    // big problems: the narrow products (heads, first decoder layer) get launches of their own, or their presence
    // would hold the wide ones on 64x64 tiles (finish_launch picks one tile shape per launch)
    auto is_narrow = [](const WorkItem& w) { return w.N <= 64 || w.M <= 64 || w.conv > 0; };    // (implicit patch matrices: small tiles only)
    auto wgrad_launches = [&](const std::vector<WorkItem>& set, std::vector<Launch>& dst, const std::string& prefix) {
        long wide128 = 0;
        for (const WorkItem& w : set) if (!is_narrow(w)) wide128 += (long)((w.M + 127) / 128) * ((w.N + 127) / 128);
        std::vector<std::vector<WorkItem>> chunks;
        auto chunk_up = [&](const std::vector<WorkItem>& v) {
            for (size_t i0 = 0; i0 < v.size(); i0 += kMaxTnItems)
                chunks.emplace_back(v.begin() + i0, v.begin() + std::min(v.size(), i0 + (size_t)kMaxTnItems));
        };
        if (wide128 >= 192) {
            std::vector<WorkItem> wide, narrow;
            for (const WorkItem& w : set) (is_narrow(w) ? narrow : wide).push_back(w);
            chunk_up(wide); chunk_up(narrow);
        } else {
            chunk_up(set);
        }
        for (size_t c = 0; c < chunks.size(); ++c) {
            group(prefix + (chunks.size() > 1 ? std::to_string(c + 1) : std::string()), dst,
                  [&] { for (const WorkItem& w : chunks[c]) h->items.push_back(w); });
        }
    };
    wgrad_launches(wg, h->wgrad, "wgrad");
    // the same weight gradients cut into the two data-parallel buckets (MLP-only models)
    h->wgrad_b[0].clear(); h->wgrad_b[1].clear();
    dp_ranges(h, &h->n_buckets, h->ranges_b);
    if (h->n_buckets == 2) {
        std::vector<WorkItem> set[2];
        for (Mod& md : h->mods) {
            set[0].push_back(bd.wgrad(md.D.back(), md.outl, md.dO));
            for (int k = md.L - 1; k >= 1; --k) set[0].push_back(bd.wgrad(md.D[k - 1], md.dec[k], md.dD[k]));
            set[0].push_back(bd.wgrad(md.Z, md.dec[0], md.dD[0]));
            set[1].push_back(bd.wgrad(md.E.back(), md.head, md.dH));
            for (int k = md.L - 1; k >= 1; --k) set[1].push_back(bd.wgrad(md.E[k - 1], md.enc[k], md.dE[k]));
            set[1].push_back(bd.wgrad(md.X0, md.enc[0], md.dE[0]));
        }
        wgrad_launches(set[0], h->wgrad_b[0], "wgrad_dec");
        wgrad_launches(set[1], h->wgrad_b[1], "wgrad_enc");
    }
    for (int i = 1; i <= 3; ++i) if (any_thin(h, i)) thin_launch(h, bd, "conv_dec" + std::to_string(i + 1) + "_wgrad_direct", h->wgrad, 2, i);
    {   // bias gradients of the adjoint-frame stages = column sums of their output gradient, first level
        Launch L;
        L.name = "conv_bias_rowsum"; L.type = kRowsum;
        int base = 0;
        for (Mod& md : h->mods) if (md.conv) for (const ConvStage& st : md.cdec) if (st.adj && !st.impl_w) {
            RowsumSeg& g = L.rs.seg[L.rs.n_seg++];
            g.src = h->at<void>(st.dY.rm); g.part = h->at<float>(st.rs_part); g.ld = st.dY.ld;
            g.rows = h->B * st.g.OH * st.g.OW; g.cols = st.d.out; g.cols4 = st.rs_cols4; g.n_blocks = kRowsumBlocks;
            g.cpow = 4; while (g.cpow < g.cols4) g.cpow *= 2;
            if (g.cpow > 64) throw Err("internal error: bias row sums hold at most 64 columns");
            g.block_base = base; base += kRowsumBlocks;
        }
        L.blocks = base;
        if (base > 0) h->wgrad.push_back(L);
    }
    {   // ... and its per-image partial sums -> the gradient buffer (one column of the padded matrix)
        Launch R;
        R.name = "conv_wgrad_sums"; R.type = kColsum;
        int base = 0;
        for (Mod& md : h->mods) if (md.conv) for (const ConvStage& st : md.cdec) if (st.adj && !st.impl_w) {      // second level of the row sums
            ReduceSeg& g = R.ra.seg[R.ra.n_seg++];
            g.dst = h->grad() + st.d.master + (size_t)st.d.in * st.d.ld; g.src = h->at<float>(st.rs_part);
            g.n = st.d.out; g.parts = kRowsumBlocks; g.stride = st.rs_cols4; g.dst_ld = 1;
            g.block_base = base; base += (g.n + 3) / 4;
        }
        for (Mod& md : h->mods) if (md.conv) for (const ConvStage& st : md.cdec) if (st.thin) {
            ReduceSeg& g = R.ra.seg[R.ra.n_seg++];
            g.dst = h->grad() + st.d.master; g.src = h->at<float>(st.thin_part);
            g.n = st.d.in + 1; g.parts = st.thin_blocks; g.stride = st.thin_kp; g.dst_ld = st.d.ld;
            g.block_base = base; base += (g.n + 3) / 4;
        }
        R.blocks = base;
        for (int i = 0; i < R.ra.n_seg; ++i) { R.ra.seg[i].colsum = 1; R.ra.seg[i].perm_k = 0; }
        if (base > 0) h->wgrad.push_back(R);
    }
    {   // the split-K slices of the conv stages' weight gradients -> the gradient buffer, in fixed order
        Launch R;
        R.name = "wgrad_reduce"; R.type = kReduce;
        int base = 0;
        // (the column sums above write other destinations: when both exist they share one launch, k_sums)
        Launch* prev = (!h->wgrad.empty() && h->wgrad.back().type == kColsum && !h->sw.no_sums_merge) ? &h->wgrad.back() : nullptr;
        if (prev) { R = *prev; R.name = prev->name + "+wgrad_reduce"; R.type = kSums; base = prev->blocks; }
        for (const WorkItem& w : wg) if (w.ksplit > 1) {
            if (R.ra.n_seg >= kMaxReduceSegs) throw Err("internal error: too many split weight gradients");
            ReduceSeg& g = R.ra.seg[R.ra.n_seg++];
            g.dst = reinterpret_cast<float*>(w.out0); g.src = reinterpret_cast<const float*>(w.out1);
            g.n = w.M * w.ld0; g.parts = w.ksplit; g.stride = (long long)w.M * w.ld0;
            g.colsum = 0; g.perm_k = 0;
            // an adjoint-frame filter gradient: its slice sums go straight into the gradient buffer's layout (no k_gperm pass)
            if (!h->sw.no_sums_merge)
                for (Mod& md : h->mods) if (md.conv) for (const ConvStage& st : md.cdec) if (st.adj && st.aksplit > 1 && g.dst == h->at<float>(st.Gadj)) {
                    g.dst = h->grad() + st.d.master;
                    g.perm_k = st.g.k; g.perm_cin = st.g.Cin; g.perm_cout = st.d.out; g.perm_ldga = st.ldga; g.perm_ld = st.d.ld;
                }
            g.block_base = base; base += (g.n / 4 + kThreads - 1) / kThreads;
        }
        R.blocks = base;
        if (prev && base > prev->blocks) *prev = R;              // merged: replaces the column-sum launch
        else if (!prev && base > 0) h->wgrad.push_back(R);
    }
    {   // adjoint-frame filter gradients -> the gradient buffer's layout
        Launch L;
        L.name = "conv_wgrad_perm"; L.type = kGperm;
        int base = 0;
        for (Mod& md : h->mods) if (md.conv) for (const ConvStage& st : md.cdec) if (st.adj && !st.impl_w) {
            if (st.aksplit > 1 && !h->sw.no_sums_merge) continue;      // permuted by its slice sum (ReduceSeg::perm_*)
            GpermSeg& g = L.gp.seg[L.gp.n_seg++];
            g.Gadj = h->at<float>(st.Gadj); g.G = h->grad() + st.d.master; g.ldga = st.ldga; g.ld = st.d.ld;
            g.k = st.g.k; g.Cin = st.g.Cin; g.Cout = st.d.out;
            g.block_base = base; base += (st.g.Cin * st.g.k * st.g.k * st.d.out + kThreads - 1) / kThreads;
        }
        L.blocks = base;
        if (base > 0) h->wgrad.push_back(L);
    }
}

// Small nets: the optimiser in the epilogue of the (single) weight-gradient launch.  Only for the plain single-replica step
// (under data parallelism the all-reduce sits between the two; avae_dp_backward / avae_dp_apply keep them apart as well).
void fuse_adam(avae_handle* h, bool any_conv) {
    h->wgrad_adam.clear();
    if (!any_conv && h->wgrad.size() == 1 && h->wgrad[0].tn && h->wgrad[0].cfg == k64x64 && h->wgrad[0].targs.xcd_group == 1
        && !h->sw.no_lean && !h->sw.no_adam_fuse) {
        Launch L = h->wgrad[0];
        bool ok = true;
        for (int i = 0; i < L.targs.n_items && ok; ++i) {
            TnItem& t = L.targs.items[i];
            ok = t.ksplit <= 1 && t.bias_row == 0 && t.K > 0;
            const Dense* dm = nullptr;
            for (const Mod& md : h->mods) {
                auto look = [&](const Dense& d) { if (h->grad() + d.master == t.out) dm = &d; };
                for (const Dense& d : md.enc) look(d);
                look(md.head);
                for (const Dense& d : md.dec) look(d);
                look(md.outl);
            }
            ok = ok && dm && t.M == dm->in + 1 && t.N == dm->out && t.ld0 == dm->ld;
            if (ok) { t.W = h->at<void>(dm->W); t.Wt = h->at<void>(dm->Wt); t.ldw = dm->ldw; t.ldt = dm->ldt; }
        }
        if (ok) {
            L.cfg = kLeanTnAdam; L.name = "wgrad+adam";
            L.targs.adam = 1;
            L.targs.d_theta = h->at<float>(h->off_theta) - h->grad();
            L.targs.d_m = h->at<float>(h->off_m) - h->grad();
            L.targs.d_v = h->at<float>(h->off_v) - h->grad();
            L.targs.beta1 = h->cfg.beta1; L.targs.beta2 = h->cfg.beta2; L.targs.eps = h->cfg.adam_eps;
            L.targs.st = h->state();
            if (!h->sw.no_xcd_pieces) xcd_pieces(L);
            h->wgrad_adam.push_back(L);
        }
    }
}

// Weight warm-up: a launch on the 8-wave NT tiles pulls the weight panels of the next grouped NT launch into the Infinity
// Cache (see k_grouped); forward and backward form one sequence (the step graph runs them back to back)
void plan_weight_warmup(avae_handle* h) {
    std::vector<Launch*> seq;
    for (Launch& L : h->plain.fwd) seq.push_back(&L);
    for (Launch& L : h->bwd) seq.push_back(&L);
    for (size_t i = 0; i < seq.size(); ++i) {
        Launch& L = *seq[i];
        if (L.type != kGrouped || L.tn || !tile_geom(L.cfg).waves8) continue;
        for (size_t j = i + 1; j < seq.size(); ++j) {
            const Launch& Nx = *seq[j];
            if (Nx.type != kGrouped) continue;               // helper launches of the conv branch in between
            if (Nx.tn) break;
            for (int k = 0; k < Nx.args.n_items && L.args.n_pf < kMaxPf; ++k) {
                const WorkItem& w = Nx.args.items[k];
                if (!is_gemm(w.kind) || w.kind == K_WGRAD) continue;
                const long bytes = (long)w.N * w.ldb * h->es;          // B = weight shadow: N rows of ldb elements
                if (bytes < 128 * 1024) continue;                     // small panels come with the first tile anyway
                L.args.pf_ptr[L.args.n_pf] = w.B; L.args.pf_lines[L.args.n_pf] = (int)(bytes / 128); ++L.args.n_pf;
            }
            break;
        }
    }
}

// The training plan's Adam tiles: one item per dense layer / conv stage, and the bucket-ordered copy of the data-parallel step.
void build_adam_tables(avae_handle* h) {
    h->adam_items.clear();
    int base = 0;
    auto add = [&](const Dense& d) {
        AdamItem a;
        std::memset(&a, 0, sizeof(a));
        a.theta = h->at<float>(h->off_theta) + d.master;
        a.m = h->at<float>(h->off_m) + d.master;
        a.v = h->at<float>(h->off_v) + d.master;
        a.g = h->grad() + d.master;
        a.W = h->at<void>(d.W); a.Wt = h->at<void>(d.Wt);
        a.rows = d.in + 1; a.cols = d.out; a.ld = d.ld; a.ldw = d.ldw; a.ldt = d.ldt;
        a.tiles_r = (a.rows + kAdamRows - 1) / kAdamRows; a.tiles_c = (a.cols + 63) / 64; a.tile_base = base;
        base += a.tiles_r * a.tiles_c;
        h->adam_items.push_back(a);
    };
    for (const Mod& md : h->mods) {
        if (md.conv) {
            for (const std::vector<ConvStage>* side : {&md.cenc, &md.cdec})
                for (const ConvStage& st : *side) {
                    add(st.d);
                    // adjoint filter shadows by the same pass (no k_wadj launch): the implicit input gradients' B operand, and -- round 2's
                    // adjoint-frame route -- the forward scatter product's
                    if ((st.adj && !h->sw.no_wadj_fold) || st.impl_bwd) {
                        AdamItem& a = h->adam_items.back();
                        a.Wadj = h->at<void>(st.Wadj); a.ldadj = st.ldadj; a.adj_k = st.g.k; a.adj_cin = st.g.Cin;
                        if (st.adj) { a.Wf = h->at<void>(st.Wf); a.ldf = st.ldf; }
                    }
                }
            continue;
        }
        for (const Dense& d : md.enc) add(d);
        add(md.head);
        for (const Dense& d : md.dec) add(d);
        add(md.outl);
    }
    h->adam_blocks = base;
    // bucket-ordered copy: per modality the items are [enc x L, head, dec x L, out]
    h->adam_items_b.clear();
    for (int bk = 0; bk < 2; ++bk) {
        h->adam_first_b[bk] = (int)h->adam_items_b.size();
        int tb = 0;
        size_t i = 0;
        for (const Mod& md : h->mods) {
            const size_t n_enc = md.conv ? md.cenc.size() : (size_t)md.L + 1, n_all = md.conv ? md.cenc.size() + md.cdec.size() : 2 * (size_t)md.L + 2;
            for (size_t k = 0; k < n_all; ++k) {
                const int which = h->n_buckets == 1 ? 0 : (k < n_enc ? 1 : 0);
                if (which == bk) {
                    AdamItem a = h->adam_items[i + k];
                    a.tile_base = tb; tb += a.tiles_r * a.tiles_c;
                    h->adam_items_b.push_back(a);
                }
            }
            i += n_all;
        }
        h->adam_count_b[bk] = (int)h->adam_items_b.size() - h->adam_first_b[bk];
        h->adam_blocks_b[bk] = tb;
    }
}

void build_training_plan(avae_handle* h) {
    h->items.clear(); h->plain.fwd.clear(); h->bwd.clear(); h->wgrad.clear(); h->conv_tab.clear();
    Builder bd(h, h->items, h->B, true);
    Groups group{h, h->items};
    int Lmax = 0;
    for (const Mod& md : h->mods) Lmax = std::max(Lmax, md.L);
    bool any_conv = false;
    for (const Mod& md : h->mods) any_conv = any_conv || md.conv;
    // ---- forward.  Modalities with fewer hidden layers simply sit out a launch; data dependencies
    // are per modality and launches are stream-ordered, so this is always safe.
    for (int k = 0; k < Lmax; ++k)
        group("fwd_enc" + std::to_string(k + 1), h->plain.fwd, [&] {
            for (Mod& md : h->mods) if (k < md.L) h->items.push_back(bd.fwd_hidden(k == 0 ? md.X0 : md.E[k - 1], md.enc[k], md.E[k]));
        });
    if (h->sw.chain2 && !any_conv) chain_enc12(h);
    if (any_conv) {   // conv encoder: three convs, then the flatten + dense heads.  Per modality and stage: implicit GEMM (the patch
                      // matrix is gathered by the GEMM's own operand loads), or im2col launch + GEMM where the channels are no whole chunks
        for (int i = 0; i < 3; ++i) {
            auto src_of = [&, i](Mod& md) { return i == 0 ? h->at<void>(md.X0.rm) : h->at<void>(md.cenc[i - 1].Y.rm); };
            gather_launch(h, bd, "conv_enc" + std::to_string(i + 1) + "_im2col", h->plain.fwd, [&](Mod& md) -> const ConvStage& { return md.cenc[i]; },
                          src_of, [i](const Mod& md) { return !md.cenc[i].impl; });
            group("conv_enc" + std::to_string(i + 1), h->plain.fwd, [&] {
                for (Mod& md : h->mods) if (md.conv) h->items.push_back(md.cenc[i].impl ? bd.conv_fwd_impl(md.cenc[i], src_of(md)) : bd.conv_fwd(md.cenc[i])); });
        }
        gather_launch(h, bd, "conv_head_im2col", h->plain.fwd, [&](Mod& md) -> const ConvStage& { return md.cenc[3]; },
                      [&](Mod& md) { return h->at<void>(md.cenc[2].Y.rm); }, [](const Mod& md) { return !md.cenc[3].impl; });
    }
    group("fwd_head", h->plain.fwd, [&] { for (Mod& md : h->mods) h->items.push_back(bd.fwd_head(md, true, md.conv && md.cenc[3].impl)); });
    // KL + association terms and their (mu, lv) gradients need every modality's (mu, lv) (ready after fwd_head) and are needed by
    // bwd_dec1_latent.  Small nets: they ride in the fwd_out_loss launch (the decoder's hidden launches stay plain GEMM launches).
    // Big nets, whose loss launch runs one 144-KB workgroup per CU on the 8-wave tile: there the item's workgroups would each take a
    // CU's only slot and send the launch into a second round (C4: 512 workgroups, 33 us), so it gets a launch of its own here.
    bool latent_alone = false;
    {
        long t64 = 0, t128 = 0;
        bool narrow = false;
        for (const Mod& md : h->mods) {
            t64 += (long)((h->B + 255) / 256) * ((md.n_in + 63) / 64);
            t128 += (long)((h->B + 127) / 128) * ((md.n_in + 127) / 128);
            narrow = narrow || md.n_in <= 64 || h->B <= 64;
        }
        latent_alone = t64 >= 192 && t128 >= 192 && !narrow && !h->sw.no_loss8;      // = choose_cfg's choice of k256x64Loss
    }
    if (latent_alone) group("latent", h->plain.fwd, [&] { h->items.push_back(bd.latent()); });
    for (int k = 0; k < std::max(Lmax, 1); ++k) {
        group("fwd_dec" + std::to_string(k + 1), h->plain.fwd, [&] {
            for (Mod& md : h->mods) if (k < md.L) h->items.push_back(bd.fwd_hidden(k == 0 ? md.Z : md.D[k - 1], md.dec[k], md.D[k]));
        });
        if (k == 0 && !any_conv && !latent_alone) fuse_tail(h, h->plain.fwd, 1);      // fwd_dec1 rides in fwd_head
    }
    if (any_conv) {   // adjoint filter shadows of the transposed-conv stages that run through Padj / the scatter product (refreshed once per step)
        Launch L;
        L.name = "conv_wadj"; L.type = kWadj;
        int base = 0;
        for (Mod& md : h->mods) if (md.conv) for (const ConvStage& st : md.cdec) if (st.adj) {
            WadjSeg& g = L.wa.seg[L.wa.n_seg++];
            g.Wt = h->at<void>(st.d.Wt); g.Wadj = h->at<void>(st.Wadj); g.Wf = h->at<void>(st.Wf); g.ldt = st.d.ldt; g.ldadj = st.ldadj; g.ldf = st.ldf;
            g.k = st.g.k; g.Cin = st.g.Cin; g.Cout = st.d.out;
            g.block_base = base; base += (st.g.Cin * st.g.k * st.g.k * st.d.out + kThreads - 1) / kThreads;
        }
        L.blocks = base;
        if (base > 0 && h->sw.no_wadj_fold) h->plain.fwd.push_back(L);       // default: k_adam writes these shadows (AdamItem::Wadj)
    }
    if (any_conv) {   // deconv decoder: four transposed convs (+ bias + sigmoid each), then the dense output layer
        for (int i = 0; i < 4; ++i) {
            // every modality routes its stage i on its own (depths differ between modalities): direct (one output channel), implicit
            // GEMM in gather form, round 2's adjoint-frame scatter product, or im2col + GEMM
            auto plain = [&, i](const Mod& md) { return !md.cdec[i].thin && !md.cdec[i].adj && !md.cdec[i].impl; };
            auto src_of = [&, i](Mod& md) { return i == 0 ? h->at<void>(md.Z.rm) : h->at<void>(md.cdec[i - 1].Y.rm); };
            if (any_thin(h, i)) thin_launch(h, bd, "conv_dec" + std::to_string(i + 1) + "_direct", h->plain.fwd, 0, i);
            if (any_adj(h, i)) {       // scatter product on the stage's (small) input, then overlap-add + bias + transfer function
                group("conv_dec" + std::to_string(i + 1) + "_scatter", h->plain.fwd, [&] {
                    for (Mod& md : h->mods) if (md.conv && md.cdec[i].adj) h->items.push_back(bd.adj_fwd(md.cdec[i], md.cdec[i - 1])); });
                Launch L;
                L.name = "conv_dec" + std::to_string(i + 1) + "_overlap"; L.type = kCol2im;
                int base = 0;
                for (Mod& md : h->mods) if (md.conv && md.cdec[i].adj) {
                    Col2imSeg c = bd.adj_overlap_seg(md.cdec[i]);
                    c.tile_base = base; base += c.tiles_r * c.tiles_c;
                    L.ca.seg[L.ca.n_seg++] = c;
                }
                L.blocks = base;
                h->plain.fwd.push_back(L);
            }
            gather_launch(h, bd, "conv_dec" + std::to_string(i + 1) + "_im2col", h->plain.fwd, [&](Mod& md) -> const ConvStage& { return md.cdec[i]; }, src_of, plain);
            group("conv_dec" + std::to_string(i + 1), h->plain.fwd, [&] {
                for (Mod& md : h->mods) if (md.conv) {
                    if (md.cdec[i].impl) h->items.push_back(bd.conv_fwd_impl(md.cdec[i], src_of(md)));
                    else if (plain(md)) h->items.push_back(bd.conv_fwd(md.cdec[i]));
                } });
        }
        gather_launch(h, bd, "conv_out_im2col", h->plain.fwd, [&](Mod& md) -> const ConvStage& { return md.cdec[4]; },
                      [&](Mod& md) { return h->at<void>(md.cdec[3].Y.rm); }, [](const Mod& md) { return !md.cdec[3].dense_map; });
    }
    group("fwd_out_loss", h->plain.fwd, [&] {
        for (int m = 0; m < h->M; ++m) h->items.push_back(bd.fwd_out(h->mods[m], m, true));
        if (!latent_alone) h->items.push_back(bd.latent());
    });
    // ---- backward: the dgrad chain (one launch per layer, all modalities), then EVERY weight gradient in the last
    // launch(es), then k_adam.  Conv stages go GEMM (fp32 patch gradients) -> k_col2im (sum + act' -> gradient of the
    // producing stage).
    group("bwd_out", h->bwd, [&] {
        for (Mod& md : h->mods) {
            if (md.conv && md.cdec[3].dense_map) {      // the 28x28 map is a dense row: an ordinary dense dgrad, sigmoid' of the stored map
                const ConvStage& s3 = md.cdec[3];
                WorkItem w = bd.dgrad_hidden(md.dO, md.outl, s3.Y, s3.dY);
                w.act = s3.act;
                h->items.push_back(w);
            }
            else if (md.conv) h->items.push_back(bd.conv_dgrad(md.cdec[4], md.dO));
            else h->items.push_back(bd.dgrad_hidden(md.dO, md.outl, md.D.back(), md.dD.back()));
        }
    });
    bool latent_conv_impl = false;          // some conv modality's first decoder stage takes the implicit latent dgrad (rides in bwd_dec1_latent)
    if (any_conv) {
        for (int i = 4; i >= 1; --i) {       // stage i's patch gradients -> dY of stage i-1; then stage i-1's input gradient
            // (per modality; a direct, adjoint-frame or implicit stage has no patch gradients: its own launch wrote the producing stage's gradient)
            auto explicit_i = [&, i](const Mod& md) { return !md.cdec[i].thin && !md.cdec[i].adj && !md.cdec[i].impl_bwd && !(i == 4 && md.cdec[3].dense_map); };
            auto plain_j = [&, i](const Mod& md) { return !md.cdec[i - 1].thin && !md.cdec[i - 1].adj && !md.cdec[i - 1].impl_bwd; };
            col2im_launch(h, bd, "conv_dec" + std::to_string(i) + "_col2im", h->bwd, [&](Mod& md) -> const ConvStage& { return md.cdec[i]; },
                          [&](Mod& md) -> const ConvStage* { return &md.cdec[i - 1]; }, explicit_i);
            if (any_thin(h, i - 1)) thin_launch(h, bd, "conv_bwd_dec" + std::to_string(i) + "_direct", h->bwd, 1, i - 1);
            if (any_adj(h, i - 1)) {     // patch matrix of stage i-1's output gradient -> GEMM with the adjoint filter -> dY of stage i-2
                Launch L;
                L.name = "conv_bwd_dec" + std::to_string(i) + "_adj_im2col"; L.type = kGather;
                int base = 0;
                for (Mod& md : h->mods) if (md.conv && md.cdec[i - 1].adj && (!md.cdec[i - 1].impl_bwd || !md.cdec[i - 1].impl_w)) {      // (Padj feeds the adjoint dgrad and the adjoint-frame filter gradient)
                    GatherSeg g = bd.adj_gather_seg(md.cdec[i - 1]);
                    g.tile_base = base; base += g.tiles_r * g.tiles_c;
                    L.ga.seg[L.ga.n_seg++] = g;
                }
                L.blocks = base;
                if (base > 0) h->bwd.push_back(L);
                group("conv_bwd_dec" + std::to_string(i) + "_adj", h->bwd, [&] {
                    for (Mod& md : h->mods) if (md.conv && md.cdec[i - 1].adj && !md.cdec[i - 1].impl_bwd) h->items.push_back(bd.adj_dgrad(md.cdec[i - 1], md.cdec[i - 2])); });
            }
            group("conv_bwd_dec" + std::to_string(i), h->bwd, [&] {
                for (Mod& md : h->mods) if (md.conv) {
                    const ConvStage& st = md.cdec[i - 1];
                    if (st.impl_bwd && i - 1 >= 1)          // implicit GEMM on stage i-1's own output gradient: writes dY of stage i-2
                        h->items.push_back(bd.adj_dgrad_impl(st, h->at<void>(st.dY.rm), st.g.OH * st.g.OW * st.dY.ld, st.dY.ld, md.cdec[i - 2].act, md.cdec[i - 2].Y, md.cdec[i - 2].dY));
                    else if (st.impl_bwd) latent_conv_impl = true;
                    else if (plain_j(md)) h->items.push_back(bd.conv_dgrad(st, st.dY));
                } });
        }
        // first decoder stage: its input is z -> latent mode turns dz into [dmu | dlv]
        col2im_launch(h, bd, "conv_dec1_latent", h->bwd, [&](Mod& md) -> const ConvStage& { return md.cdec[0]; },
                      [&](Mod&) -> const ConvStage* { return nullptr; }, [](const Mod& md) { return !md.cdec[0].impl_bwd; });
    }
    for (int k = Lmax - 1; k >= 1; --k)
        group("bwd_dec" + std::to_string(k + 1), h->bwd, [&] {
            for (Mod& md : h->mods) if (k < md.L) h->items.push_back(bd.dgrad_hidden(md.dD[k], md.dec[k], md.D[k - 1], md.dD[k - 1]));
        });
    group("bwd_dec1_latent", h->bwd, [&] {
        for (Mod& md : h->mods) {
            if (!md.conv) h->items.push_back(bd.dgrad_latent(md));
            else if (md.cdec[0].impl_bwd) h->items.push_back(bd.adj_dgrad_latent_impl(md.cdec[0], md));
        }
        h->items.push_back(bd.cost(true));                       // every cost partial is final since fwd_out_loss: cost, step counter, lr_t
    });
    (void)latent_conv_impl;
    h->bwd_split = (int)h->bwd.size();      // everything from here on belongs to the encoder side
    group("bwd_head", h->bwd, [&] {
        for (Mod& md : h->mods) {
            if (md.conv && md.cenc[3].impl_bwd)     // implicit: the heads' input gradient straight into the 3x3 map's gradient rows
                h->items.push_back(bd.adj_dgrad_impl(md.cenc[3], h->at<void>(md.dH.rm), md.dH.ld, md.dH.ld, md.cenc[2].act, md.cenc[2].Y, md.cenc[2].dY));
            else if (md.conv) h->items.push_back(bd.conv_dgrad(md.cenc[3], md.dH));
            else h->items.push_back(bd.dgrad_hidden(md.dH, md.head, md.E.back(), md.dE.back()));
        }
    });
    if (!any_conv) fuse_tail(h, h->bwd, 2);                                      // bwd_head rides in bwd_dec1_latent
    if (any_conv) {
        for (int i = 3; i >= 1; --i) {
            col2im_launch(h, bd, "conv_enc" + std::to_string(i) + "_col2im", h->bwd, [&](Mod& md) -> const ConvStage& { return md.cenc[i]; },
                          [&](Mod& md) -> const ConvStage* { return &md.cenc[i - 1]; }, [i](const Mod& md) { return !md.cenc[i].impl_bwd; });
            if (i >= 2) group("conv_bwd_enc" + std::to_string(i), h->bwd, [&] {
                for (Mod& md : h->mods) if (md.conv) {
                    const ConvStage& st = md.cenc[i - 1];
                    if (st.impl_bwd) h->items.push_back(bd.adj_dgrad_impl(st, h->at<void>(st.dY.rm), st.g.OH * st.g.OW * st.dY.ld, st.dY.ld, md.cenc[i - 2].act, md.cenc[i - 2].Y, md.cenc[i - 2].dY));
                    else h->items.push_back(bd.conv_dgrad(st, st.dY));
                } });
        }
    }
    for (int k = Lmax - 1; k >= 1; --k) {
        group("bwd_enc" + std::to_string(k + 1), h->bwd, [&] {
            for (Mod& md : h->mods) if (k < md.L) h->items.push_back(bd.dgrad_hidden(md.dE[k], md.enc[k], md.E[k - 1], md.dE[k - 1]));
        });
    }
    if (any_conv && !h->sw.no_sink) sink_and_hoist(h);
    plan_weight_gradients(h, bd, group);
    fuse_adam(h, any_conv);
    if (!h->sw.no_warm) plan_weight_warmup(h);
    // ---- eval: forward launches + a lone cost reduction that does not bump the step
    {
        const int first = (int)h->items.size();
        h->items.push_back(bd.cost(false));
        h->cost_only = finish_launch(h, h->items, first, 1, "cost_reduce", &group.slot);
    }
    build_adam_tables(h);
}

void build_inference(avae_handle* h, int m, bool enc, int rows) {
    avae_handle::Inf& inf = enc ? h->inf_enc[m] : h->inf_dec[m];
    if (inf.rows == rows) return;
    inf.items.clear(); inf.launches.clear();
    Builder bd(h, inf.items, rows, false);
    Mod& md = h->mods[m];
    int slot = 0;
    auto one = [&](const WorkItem& w, const std::string& name) {
        inf.items.push_back(w);
        inf.launches.push_back(finish_launch(h, inf.items, (int)inf.items.size() - 1, 1, name, &slot));
    };
    auto gather1 = [&](const ConvStage& st, const void* src, const std::string& name) {
        Launch L;
        L.name = name; L.type = kGather;
        GatherSeg g = bd.gather_seg(st, src);
        g.tile_base = 0;
        L.ga.seg[0] = g; L.ga.n_seg = 1;
        L.blocks = g.tiles_r * g.tiles_c;
        inf.launches.push_back(L);
    };
    if (enc && md.conv) {
        for (int i = 0; i < 3; ++i) {
            gather1(md.cenc[i], i == 0 ? h->at<void>(md.X0.rm) : h->at<void>(md.cenc[i - 1].Y.rm), "inf_conv_im2col");
            one(bd.conv_fwd(md.cenc[i]), "inf_conv_enc");
        }
        gather1(md.cenc[3], h->at<void>(md.cenc[2].Y.rm), "inf_conv_im2col");
        one(bd.fwd_head(md, true), "inf_head");
    } else if (enc) {
        for (int k = 0; k < md.L; ++k) one(bd.fwd_hidden(k == 0 ? md.X0 : md.E[k - 1], md.enc[k], md.E[k]), "inf_enc");
        one(bd.fwd_head(md, true), "inf_head");
    } else if (md.conv) {
        for (int i = 0; i < 4; ++i) {
            if (md.cdec[i].dense_map) {      // the one-channel 28x28 stage writes dense rows: the direct kernel, as in training
                Launch L;
                L.name = "inf_conv_dec_direct"; L.type = kThin;
                L.ta.mode = 0;
                ThinSeg t = bd.thin_seg(md.cdec[i], md.cdec[i - 1]);
                t.block_base = 0;
                L.ta.seg[0] = t; L.ta.n_seg = 1;
                L.blocks = rows * t.split;
                inf.launches.push_back(L);
                continue;
            }
            gather1(md.cdec[i], i == 0 ? h->at<void>(md.Z.rm) : h->at<void>(md.cdec[i - 1].Y.rm), "inf_conv_im2col");
            one(bd.conv_fwd(md.cdec[i]), "inf_conv_dec");
        }
        if (!md.cdec[3].dense_map) gather1(md.cdec[4], h->at<void>(md.cdec[3].Y.rm), "inf_conv_im2col");
        one(bd.fwd_out(md, m, false), "inf_out");
    } else {
        for (int k = 0; k < md.L; ++k) one(bd.fwd_hidden(k == 0 ? md.Z : md.D[k - 1], md.dec[k], md.D[k]), "inf_dec");
        one(bd.fwd_out(md, m, false), "inf_out");
    }
    inf.rows = rows;
}

// ----------------------------------------------------------------------------- execution
int tname_id(avae_handle* h, const std::string& n) {
    for (size_t i = 0; i < h->tnames.size(); ++i) if (h->tnames[i] == n) return (int)i;
    h->tnames.push_back(n);
    return (int)h->tnames.size() - 1;
}

struct Timed {
    avae_handle* h; hipStream_t s; bool on; hipEvent_t a = nullptr, b = nullptr; int id = 0;
    Timed(avae_handle* h_, hipStream_t s_, const std::string& name) : h(h_), s(s_), on(h_->timing && h_->trecs.size() < 200000) {
        if (!on) return;
        id = tname_id(h, name);
        HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b));
        t_launch_events = LaunchEvents{a, b};         // the launch inside this scope stamps them with its own begin/end
    }
    ~Timed() {
        if (!on) return;
        if (t_launch_events.start) {                  // nothing was launched (empty segment): record an empty bracket
            t_launch_events = LaunchEvents{nullptr, nullptr};
            (void)hipEventRecord(a, s); (void)hipEventRecord(b, s);
        }
        h->trecs.push_back(TimingRec{a, b, id});
    }
};

// One kernel launch outside the plans' tables: its timing bracket, the launch, its error check -- both under `name`.
template <typename F> void timed_launch(avae_handle* h, hipStream_t s, const char* name, F&& launch) {
    Timed t(h, s, name);
    launch();
    LAUNCH_OK(name);
}

// The same launch reading staging set j instead of set 0: every pointer into set 0 moves by j * stage_bytes.  hyper (a scheduled
// training step): its latent and cost items read entry j of the schedule table.
Launch relocated(const avae_handle* h, const Launch& L0, int j, const HyperEntry* hyper = nullptr) {
    Launch L = L0;
    const unsigned char* lo = h->ws + h->stage_lo;
    const unsigned char* hi = lo + h->stage_bytes;
    const size_t delta = (size_t)j * h->stage_bytes;
    auto fix = [&](auto& ptr) {
        const unsigned char* q = reinterpret_cast<const unsigned char*>(ptr);
        if (q >= lo && q < hi) ptr = reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(const_cast<unsigned char*>(q) + delta);
    };
    for (int i = 0; i < L.args.n_items && L.type == kGrouped; ++i) {
        WorkItem& w = L.args.items[i];
        fix(w.A); fix(w.B); fix(w.out0); fix(w.out1); fix(w.out2); fix(w.aux0); fix(w.aux1); fix(w.aux2); fix(w.eps);
        fix(w.tail_w); fix(w.tail_out); fix(w.tail_aux);
        if (w.present) w.present += (size_t)j * h->pres_set;          // masked twin: presence set j (its own allocation)
        if (hyper && (w.kind == K_LATENT || (w.kind == K_COST && w.bump_step))) w.tail_w = hyper + j;
    }
    for (int i = 0; i < L.targs.n_items && L.type == kGrouped; ++i) { TnItem& t = L.targs.items[i]; fix(t.A); fix(t.B); fix(t.out); }
    for (int i = 0; i < L.ga.n_seg && L.type == kGather; ++i) fix(L.ga.seg[i].src);
    L.desc_set = j;
    return L;
}

// Deals the tiles that the by-value kernels run on XCD p (lists[p], in their order there) into ONE order in which record x runs on
// XCD x % 8 with exactly as many records as tiles: where an XCD's list is shorter than the others', the hole takes a tile from the
// end of a longer one.
template <typename D> std::vector<D> deal_to_xcds(const std::vector<D> (&lists)[8]) {
    size_t total = 0;
    for (const auto& l : lists) total += l.size();
    std::vector<D> out(total), spill;
    std::vector<char> set(total, 0);
    for (int p = 0; p < 8; ++p)
        for (size_t i = 0; i < lists[p].size(); ++i) {
            const size_t x = 8 * i + p;
            if (x < total) { out[x] = lists[p][i]; set[x] = 1; } else spill.push_back(lists[p][i]);
        }
    size_t k = 0;
    for (size_t x = 0; x < total; ++x) if (!set[x]) out[x] = spill[k++];
    return out;
}

// The records of one k_small launch (tile configuration 7, hidden forward or hidden dgrad items): every (item, tile) the by-value
// kernel would run, resolved as its prologue resolves it.  Empty: the launch stays on its by-value arguments.
std::vector<SmallDesc> small_descs(const avae_handle* h, const Launch& L) {
    std::vector<SmallDesc> lists[8];
    const int es = h->es;
    for (int y = 0; y < L.args.n_items; ++y) {
        const WorkItem& w = L.args.items[y];
        if (w.kind != L.args.items[0].kind || w.act != L.args.items[0].act || (w.kind != K_FWD_HIDDEN && w.kind != K_DGRAD_HIDDEN)) return {};
        const int nt = w.tiles_m * w.tiles_n, q = nt >> 3, r = nt & 7;
        for (int part = 0; part < 8; ++part)
            for (int idx = 0; idx < q + (part < r ? 1 : 0); ++idx) {
                const int t = (part < r ? part * (q + 1) : r * (q + 1) + (part - r) * q) + idx;
                const int tm = t / w.tiles_n, tn = t - tm * w.tiles_n, m0 = tm * 32, n0 = tn * 32;
                SmallDesc d{};
                d.a = static_cast<const unsigned char*>(w.A) + (size_t)m0 * w.lda * es;
                d.b = static_cast<const unsigned char*>(w.B) + (size_t)n0 * w.ldb * es;
                d.out = static_cast<unsigned char*>(w.out0) + ((size_t)m0 * w.ld0 + n0) * es;
                d.aux = w.kind == K_DGRAD_HIDDEN ? static_cast<const unsigned char*>(w.aux0) + ((size_t)m0 * w.ldx + n0) * es : nullptr;
                d.lda = w.lda; d.ldb = w.ldb; d.ld0 = w.ld0; d.ldx = w.ldx;
                d.nk = (w.K * es) / kTileBytesK;
                d.mrem = w.M - m0; d.nrem = w.N - n0; d.xrem = w.ldx - n0;
                lists[part].push_back(d);
            }
    }
    return deal_to_xcds(lists);
}

// The records of the k_small_tn launch (tile configuration 12): the tiles of XCD p are its pieces' (TnLaunchArgs::pieces), or its
// share of every entry, exactly as the by-value kernel finds them.
std::vector<TnDesc> tn_descs(const avae_handle* h, const Launch& L) {
    std::vector<TnDesc> lists[8];
    const TnLaunchArgs& a = L.targs;
    const int es = h->es;
    for (int y = 0; y < L.grid_y; ++y)
        for (int x = 0; x < L.grid_x; ++x) {
            const int part = x & 7, idx = x >> 3;
            int entry = y, t = -1;
            if (a.xcd_pieces) {
                int e = 0, lo = 0;
                for (int i = 0; i < kTnPieces; ++i) { const int ce = a.pieces[part][i].cum_end; if (idx >= ce) { e = i + 1; lo = ce; } }
                if (e >= kTnPieces) continue;
                entry = a.pieces[part][e].item; t = a.pieces[part][e].tile_off + idx - lo;
            } else {
                if (entry >= a.n_items) continue;
                const int nt = a.items[entry].tile_cnt, q = nt >> 3, r = nt & 7;
                if (idx >= q + (part < r ? 1 : 0)) continue;
                t = (part < r ? part * (q + 1) : r * (q + 1) + (part - r) * q) + idx + a.items[entry].tile_off;
            }
            const TnItem& w = a.items[entry];
            const int tm = t / w.tiles_n, tn = t - tm * w.tiles_n, m0 = tm * 64, n0 = tn * 64;
            const int nk = (w.K * es) / kTileBytesK;
            if (nk > 65535 || !w.W || !w.Wt) return {};
            TnDesc d{};
            d.a = static_cast<const unsigned char*>(w.A) + (size_t)m0 * es;
            d.b = static_cast<const unsigned char*>(w.B) + (size_t)n0 * es;
            d.out = w.out + (size_t)m0 * w.ld0 + n0;
            d.w = static_cast<unsigned char*>(w.W) + ((size_t)m0 * w.ldw + n0) * es;
            d.wt = static_cast<unsigned char*>(w.Wt) + ((size_t)n0 * w.ldt + m0) * es;
            d.lda = w.lda; d.ldb = w.ldb; d.ld0 = w.ld0; d.ldw = w.ldw; d.ldt = w.ldt;
            d.ext = TnDesc::pack(nk, w.M - m0, w.N - n0);
            lists[part].push_back(d);
        }
    return deal_to_xcds(lists);
}

// The tiles of item w that the by-value kernels run on XCD `part`, in their order there: f(t)
template <typename F> void tiles_of_part(const WorkItem& w, int part, F&& f) {
    const int nt = w.tiles_m * w.tiles_n, q = nt >> 3, r = nt & 7;
    for (int idx = 0; idx < q + (part < r ? 1 : 0); ++idx) f((part < r ? part * (q + 1) : r * (q + 1) + (part - r) * q) + idx);
}

// The records of the output + loss launch (tile configuration 9): the 32x32 tiles of its K_FWD_OUT_LOSS items as k_small_loss
// resolves them, and one record per tile of the K_LATENT item that names item and tile.  Empty (the launch stays by-value): an item
// of another kind, a masked twin's item, an implicit patch matrix.
std::vector<LossRec> loss_recs(const avae_handle* h, const Launch& L) {
    std::vector<LossRec> lists[8];
    const int es = h->es;
    for (int y = 0; y < L.args.n_items; ++y) {
        const WorkItem& w = L.args.items[y];
        if ((w.kind != K_FWD_OUT_LOSS && w.kind != K_LATENT) || w.present || w.conv > 0 || w.bias_ep) return {};
        for (int part = 0; part < 8; ++part)
            tiles_of_part(w, part, [&](int t) {
                LossRec d{};
                d.item = -1;
                if (w.kind == K_LATENT) { d.item = y; d.tile = t; lists[part].push_back(d); return; }
                const int tm = t / w.tiles_n, tn = t - tm * w.tiles_n, m0 = tm * 32, n0 = tn * 32;
                d.a = static_cast<const unsigned char*>(w.A) + (size_t)m0 * w.lda * es;
                d.b = static_cast<const unsigned char*>(w.B) + (size_t)n0 * w.ldb * es;
                d.out = static_cast<unsigned char*>(w.out0) + ((size_t)m0 * w.ld0 + n0) * es;
                d.x = static_cast<const float*>(w.aux0) + (size_t)m0 * w.ldx + n0;
                d.slot = w.partial + w.slot_base + t;
                d.lda = w.lda; d.ldb = w.ldb; d.ld0 = w.ld0; d.ldx = w.ldx;
                d.nk = (w.K * es) / kTileBytesK;
                d.mrem = w.M - m0; d.nrem = w.N - n0; d.xrem = w.ldx - n0;
                d.scale = w.scale; d.binary = w.binary;
                lists[part].push_back(d);
            });
    }
    return deal_to_xcds(lists);
}

// The records of a fused head launch: fwd_head + fwd_dec1 (tile configuration 11, K_FWD_HEAD items with a forward tail) or
// bwd_dec1_latent + bwd_head (10, K_DGRAD_LATENT items with a dgrad tail, and the step's K_COST item as a record that names it).
std::vector<HeadRec> head_recs(const avae_handle* h, const Launch& L) {
    std::vector<HeadRec> lists[8];
    const int es = h->es;
    const bool bwd = L.cfg == kLeanLatb;
    for (int y = 0; y < L.args.n_items; ++y) {
        const WorkItem& w = L.args.items[y];
        const bool cost = bwd && w.kind == K_COST;
        if (!cost && (w.kind != (bwd ? K_DGRAD_LATENT : K_FWD_HEAD) || w.tail_mode != (bwd ? 2 : 1) || w.tail_act != L.lean_act)) return {};
        if (!cost && (w.present || w.conv > 0 || w.bias_ep || w.tail_kt < 1 || w.tail_kt > 2)) return {};
        for (int part = 0; part < 8; ++part)
            tiles_of_part(w, part, [&](int t) {
                HeadRec d{};
                d.item = -1;
                if (cost) { d.item = y; lists[part].push_back(d); return; }
                const int tm = t / w.tiles_n, ts = t - tm * w.tiles_n, m0 = tm * 32;
                d.a = static_cast<const unsigned char*>(w.A) + (size_t)m0 * w.lda * es;
                d.b = static_cast<const unsigned char*>(w.B);
                d.tail_w = static_cast<const unsigned char*>(w.tail_w);
                d.tail_out = static_cast<unsigned char*>(w.tail_out) + (size_t)m0 * w.tail_ldo * es;
                if (bwd) {
                    d.out0 = static_cast<unsigned char*>(w.out0) + (size_t)m0 * w.ld0 * es;                    // dH, compute dtype
                    d.aux = static_cast<const float*>(w.aux2) + (size_t)m0 * 3 * ((w.nz + 3) & ~3);           // [g0mu | g0lv | F]
                    d.tail_aux = static_cast<const unsigned char*>(w.tail_aux) + (size_t)m0 * w.tail_ldx * es;
                } else {
                    d.out0 = static_cast<float*>(w.out0) + (size_t)m0 * w.ld0;                                // mulv, fp32
                    d.out1 = static_cast<unsigned char*>(w.out1) + (size_t)m0 * w.ld1 * es;                    // Z
                    d.aux = static_cast<const float*>(w.aux0) + (size_t)m0 * w.ldx;                           // eps
                }
                d.lda = w.lda; d.ldb = w.ldb; d.ld0 = w.ld0; d.ld1 = w.ld1; d.ldx = w.ldx;
                d.tail_ldw = w.tail_ldw; d.tail_ldo = w.tail_ldo; d.tail_ldx = w.tail_ldx;
                d.nk = (w.K * es) / kTileBytesK; d.nz = w.nz;
                d.mrem = w.M - m0; d.tail_n = w.tail_n;
                d.tk = HeadRec::pack(w.tail_kt, ts);
                lists[part].push_back(d);
            });
    }
    return deal_to_xcds(lists);
}

// Tile configurations whose training-plan launches run on two-line records (LossRec, HeadRec)
bool two_line_records(const Launch& L) { return L.type == kGrouped && !L.tn && tile_geom(L.cfg).records == 2; }

// Builds the device table of per-workgroup descriptors for the training plan's launches and points the launches at it
// (avae_device.h: SmallDesc, TnDesc, LossRec, HeadRec).  One copy of a launch's records per staging set (a record holds resolved
// addresses, and some of them point into the set).  AVAE_NO_DESC=1 keeps every launch on its by-value arguments (A/B).
void build_descriptors(avae_handle* h, hipStream_t s) {
    if (h->sw.no_desc) return;
    std::vector<unsigned char> tab;
    auto add = [&](Launch& L) {
        if (L.type != kGrouped || !((L.cfg == kLean && !L.tn) || (L.cfg == kLeanTnAdam && L.tn && L.targs.adam) || two_line_records(L))) return;
        tab.resize((tab.size() + 127) & ~(size_t)127);        // (two-line records start on an even line)
        const size_t off = tab.size();
        size_t stride = 0;
        int n = 0;
        auto put = [&](const auto& d) {                       // the records of one staging set; false: the launch stays by-value
            if (d.empty()) { tab.resize(off); return false; }
            const size_t at = tab.size(), bytes = d.size() * sizeof(d[0]);
            tab.resize(at + bytes);
            std::memcpy(tab.data() + at, d.data(), bytes);
            n = (int)d.size();
            return true;
        };
        for (int j = 0; j < kMultiSteps; ++j) {
            const Launch Lj = j == 0 ? L : relocated(h, L, j);
            const size_t at = tab.size();
            if (L.cfg == kLeanLoss) {
                if (!put(loss_recs(h, Lj))) return;
            } else if (L.cfg == kLeanLatb || L.cfg == kLeanHead) {
                if (!put(head_recs(h, Lj))) return;
            } else if (L.tn) {
                const std::vector<TnDesc> d = tn_descs(h, Lj);
                if (d.empty()) { tab.resize(off); return; }
                const TnDescArgs ca = {L.targs.d_theta, L.targs.d_m, L.targs.d_v, L.targs.beta1, L.targs.beta2, L.targs.eps, L.targs.st};
                tab.resize(at + (kTnDescHead + d.size()) * 64, 0);
                for (int p = 0; p < kTnDescHead; ++p) std::memcpy(tab.data() + at + 64 * p, &ca, sizeof(ca));
                std::memcpy(tab.data() + at + 64 * kTnDescHead, d.data(), d.size() * 64);
                n = (int)d.size();
            } else {
                const std::vector<SmallDesc> d = small_descs(h, Lj);
                if (d.empty()) { tab.resize(off); return; }
                tab.resize(at + d.size() * 64);
                std::memcpy(tab.data() + at, d.data(), d.size() * 64);
                n = (int)d.size();
            }
            stride = tab.size() - at;
        }
        L.desc_n = n; L.desc_off = off; L.desc_stride = stride;
    };
    for (Launch& L : h->plain.fwd) add(L);
    for (Launch& L : h->bwd) add(L);
    for (Launch& L : h->wgrad_adam) add(L);
    if (tab.empty()) return;
    HIP_OK(hipMemcpyAsync(h->desc_buf.ensure(tab.size()), tab.data(), tab.size(), hipMemcpyHostToDevice, s));
    HIP_OK(hipStreamSynchronize(s));      // (tab is a local)
}

template <typename D> const D* desc_of(const avae_handle* h, const Launch& L) {
    return reinterpret_cast<const D*>(h->desc_buf.as<unsigned char>() + L.desc_off + (size_t)L.desc_set * L.desc_stride);
}

// What a launch warms for the one that runs after it (next, on staging set next_set; null: nothing runs after it in this graph)
DescWarm warm_for(const avae_handle* h, const Launch* next, int next_set) {
    if (!next || next->desc_n == 0 || next_set >= kMultiSteps) return DescWarm{nullptr, 0};
    const int lines = two_line_records(*next) ? 2 * next->desc_n | kWarmPairs : next->desc_n + (next->tn ? kTnDescHead : 0);      // 64-byte lines
    return DescWarm{h->desc_buf.as<unsigned char>() + next->desc_off + (size_t)next_set * next->desc_stride, lines};
}

// One launch of a plan as the dumps print it (AVAE_DEBUG_SYNC=1: every launch that runs; AVAE_PLAN_DUMP=1: a serve plan when it is built)
void dump_launch(const Launch& L) {
    std::fprintf(stderr, "[avae] launch %s type=%d cfg=%d items=%d blocks=%d\n", L.name.c_str(), L.type, L.cfg, L.count, L.blocks);
    // runs on its records, not on the items below (two-line records: only the latent / cost item is still read from them)
    if (L.desc_n) std::fprintf(stderr, two_line_records(L) ? "        records=%d set=%d\n" : "        descriptors=%d set=%d\n", L.desc_n, L.desc_set);
    for (int i = 0; i < L.args.n_items && L.type == kGrouped; ++i)
        std::fprintf(stderr, "        item kind=%d M=%d N=%d K=%d lda=%d ldb=%d tiles=%dx%d\n", L.args.items[i].kind, L.args.items[i].M,
                     L.args.items[i].N, L.args.items[i].K, L.args.items[i].lda, L.args.items[i].ldb, L.args.items[i].tiles_m, L.args.items[i].tiles_n);
    for (int i = 0; i < L.ga.n_seg && L.type == kGather; ++i)
        std::fprintf(stderr, "        gather B=%d IH=%d Cin=%d OH=%d k=%d so=%d d=%d pad=%d sb=%d sp=%d ones=%d ldp=%d tiles=%dx%d\n", L.ga.seg[i].g.B, L.ga.seg[i].g.IH,
                     L.ga.seg[i].g.Cin, L.ga.seg[i].g.OH, L.ga.seg[i].g.k, L.ga.seg[i].g.so, L.ga.seg[i].g.d, L.ga.seg[i].g.pad, L.ga.seg[i].g.src_sb, L.ga.seg[i].g.src_sp,
                     L.ga.seg[i].g.ones, L.ga.seg[i].ldp, L.ga.seg[i].tiles_r, L.ga.seg[i].tiles_c);
    for (int i = 0; i < L.ca.n_seg && L.type == kCol2im; ++i)
        std::fprintf(stderr, "        col2im B=%d IH=%d Cin=%d OH=%d k=%d lddp=%d lda=%d g0=%p tiles=%dx%d\n", L.ca.seg[i].g.B, L.ca.seg[i].g.IH, L.ca.seg[i].g.Cin,
                     L.ca.seg[i].g.OH, L.ca.seg[i].g.k, L.ca.seg[i].lddp, L.ca.seg[i].lda, (const void*)L.ca.seg[i].g0, L.ca.seg[i].tiles_r, L.ca.seg[i].tiles_c);
}

// keep_grad = false (the descriptor wgrad+adam launch only): the launch does not store its gradient
void run_launch(avae_handle* h, const Launch& L, hipStream_t s, unsigned long long* stamps, int stamp, DescWarm warm = DescWarm{nullptr, 0},
                bool keep_grad = true) {
    Timed t(h, s, L.name);
    if (L.type == kGather) launch_gather(h->cfg.compute_dtype, L.ga, L.blocks, s);
    else if (L.type == kCol2im) launch_col2im(h->cfg.compute_dtype, L.ca, L.blocks, s);
    else if (L.type == kReduce) launch_reduce(L.ra, L.blocks, s);
    else if (L.type == kThin) launch_thin(h->cfg.compute_dtype, L.ta, L.blocks, s);
    else if (L.type == kColsum) launch_colsum(L.ra, L.blocks, s);
    else if (L.type == kWadj) launch_wadj(h->cfg.compute_dtype, L.wa, L.blocks, s);
    else if (L.type == kGperm) launch_gperm(L.gp, L.blocks, s);
    else if (L.type == kRowsum) launch_rowsum(h->cfg.compute_dtype, L.rs, L.blocks, s);
    else if (L.type == kSums) launch_sums(L.ra, L.blocks, s);
    else if (L.cfg == kChain2) launch_chain2(h->cfg.compute_dtype, L.args, L.grid_x, L.grid_y, L.lds, h->at<unsigned>(h->off_chain), h->at<unsigned>(h->off_chain) + kMaxMod * 64, s);
    else if (L.cfg == kLeanHead && L.desc_n) launch_head_rec(h->cfg.compute_dtype, L.lean_act, desc_of<HeadRec>(h, L), L.desc_n, L.lds, warm, s, stamps, stamp);
    else if (L.cfg == kLeanLatb && L.desc_n) launch_latb_rec(h->cfg.compute_dtype, L.lean_act, desc_of<HeadRec>(h, L), L.desc_n, L.lds, warm, h->state(), L.args, s, stamps, stamp);
    else if (L.cfg == kLeanLoss && L.desc_n) launch_loss_rec(h->cfg.compute_dtype, desc_of<LossRec>(h, L), L.desc_n, L.lds, warm, L.args, s, stamps, stamp);
    else if (L.cfg == kLeanHead) launch_small_head(h->cfg.compute_dtype, L.lean_act, L.args, L.grid_x, L.grid_y, L.lds, s, stamps, stamp);
    else if (L.cfg == kLeanLatb) launch_small_latb(h->cfg.compute_dtype, L.lean_act, L.args, L.grid_x, L.grid_y, L.lds, h->state(), s, stamps, stamp);
    else if (L.cfg == kLeanLoss) launch_small_loss(h->cfg.compute_dtype, L.args, L.grid_x, L.grid_y, L.lds, s, stamps, stamp);
    else if (L.cfg == kLean && L.desc_n) launch_small_desc(h->cfg.compute_dtype, L.args.items[0].kind == K_DGRAD_HIDDEN, L.args.items[0].act, desc_of<SmallDesc>(h, L), L.desc_n, L.lds, warm, s, stamps, stamp);
    else if (L.cfg == kLean) launch_small(h->cfg.compute_dtype, L.args, L.grid_x, L.grid_y, L.lds, s, stamps, stamp);
    else if (L.tn && L.cfg == kLeanTnAdam && L.desc_n) launch_small_tn_desc(h->cfg.compute_dtype, desc_of<TnDesc>(h, L), L.desc_n, keep_grad, warm, s, stamps, stamp);
    else if (L.tn && L.cfg == kLeanTnAdam) launch_small_tn(h->cfg.compute_dtype, L.targs, L.grid_x, L.grid_y, s, stamps, stamp);
    else if (L.tn) launch_grouped_tn(h->cfg.compute_dtype, L.cfg, L.targs, L.grid_x, L.grid_y, L.lds, h->state(), s, stamps, stamp);
    else launch_grouped(h->cfg.compute_dtype, L.cfg, L.args, L.grid_x, L.grid_y, L.lds, h->state(), s, stamps, stamp);
    LAUNCH_OK(L.name);
    if (h->sw.debug_sync) {      // AVAE_DEBUG_SYNC=1: name the launch a fault belongs to
        dump_launch(L);
        std::fflush(stderr);
        HIP_OK(hipStreamSynchronize(s));
    }
}

bool has_hyper_item(const Launch& L) {
    for (int i = 0; i < L.args.n_items && L.type == kGrouped; ++i)
        if (L.args.items[i].kind == K_LATENT || (L.args.items[i].kind == K_COST && L.args.items[i].bump_step)) return true;
    return false;
}

// Launches [lo, hi) of ls on staging set j: set 0 runs ls itself, set j > 0 relocated copies.  stamp_base >= 0 (AVAE_STAMPS builds):
// the launches write their clock stamps from slot stamp_base on.  train: a training step -- with a schedule set its latent and cost
// launches are copies that point at the step's schedule entry (every other caller runs the tables as they are: multipliers 1).
// after / after_set: the launch that runs behind ls[hi - 1] and its staging set -- the last launch warms its descriptors (warm_for).
// records2 = false (a masked step): the launches on two-line records run on their by-value arguments.
// keep_grad: run_launch's.
void run_set(avae_handle* h, const std::vector<Launch>& ls, size_t lo, size_t hi, int j, hipStream_t s, int stamp_base = -1, bool train = false,
             const Launch* after = nullptr, int after_set = 0, bool records2 = true, bool keep_grad = true) {
    unsigned long long* stamps = nullptr;
#ifdef AVAE_STAMPS
    if (stamp_base >= 0) stamps = h->at<unsigned long long>(h->off_stamps);
#endif
    const HyperEntry* hyper = nullptr;
    if (train && h->sched_on) {
        if (!h->sched_buf.p) throw Err("internal error: a schedule is on without its device state");
        if (j < 0 || j >= kHyperSets) throw Err("internal error: staging set outside the schedule table");
        hyper = h->sched_buf.as<SchedState>()->tab;
    }
    for (size_t i = lo; i < hi && i < ls.size(); ++i) {
        const int k = stamp_base + (int)(i - lo);
        const bool last = i + 1 >= hi || i + 1 >= ls.size();
        const DescWarm warm = last ? warm_for(h, after, after_set) : warm_for(h, &ls[i + 1], j);
        const bool strip = !records2 && ls[i].desc_n && two_line_records(ls[i]);
        if (j == 0 && !(hyper && has_hyper_item(ls[i])) && !strip) { run_launch(h, ls[i], s, stamps, k, warm, keep_grad); continue; }
        Launch L = relocated(h, ls[i], j, hyper);
        if (strip) L.desc_n = 0;
        run_launch(h, L, s, stamps, k, warm, keep_grad);
    }
}

void run_launches(avae_handle* h, const std::vector<Launch>& ls, hipStream_t s) { run_set(h, ls, 0, ls.size(), 0, s); }

// mode 0: the optimiser (with the average's update while averaging is on); mode 1: the shadows from theta, or -- from_avg -- from the average
void run_adam(avae_handle* h, int mode, hipStream_t s, int bucket = -1, bool from_avg = false) {
    AdamArgs a;
    std::memset(&a, 0, sizeof(a));
    int blocks = h->adam_blocks;
    if (bucket < 0) {
        a.items = h->at<AdamItem>(h->off_adam);
        a.n_items = (int)h->adam_items.size();
        if (a.n_items > kMaxAdamItems) throw Err("internal error: too many Adam items");
        for (int i = 0; i < a.n_items; ++i) a.base[i] = h->adam_items[i].tile_base;
    } else {
        a.items = h->at<AdamItem>(h->off_adam_b) + h->adam_first_b[bucket];
        a.n_items = h->adam_count_b[bucket];
        for (int i = 0; i < a.n_items; ++i) a.base[i] = h->adam_items_b[h->adam_first_b[bucket] + i].tile_base;
        blocks = h->adam_blocks_b[bucket];
        if (blocks == 0) return;
    }
    a.book = (bucket <= 0) ? 1 : 0;            // the bucket that carries the cost slot books the step's cost
    a.mode = mode;
    a.lr = h->cfg.learning_rate; a.beta1 = h->cfg.beta1; a.beta2 = h->cfg.beta2; a.eps = h->cfg.adam_eps;
    a.st = h->state();
    a.cost_src = h->grad() + h->P_int;
    a.clip = (mode == 0 && h->clip_on) ? h->clip_buf.as<ClipState>() : nullptr;      // the clip-aware instance (mode 1 is never clipped)
    a.n_partial = sumsq_blocks((long long)h->P_int);
    if (mode == 0 ? h->ema_on : from_avg) {          // the averaging instance
        if (!h->ema_buf.p) throw Err("internal error: averaging is on without its device state");
        a.ema = h->ema_buf.as<EmaState>(); a.avg = h->ema_avg(); a.theta0 = h->at<float>(h->off_theta);
    }
    Timed t(h, s, mode == 0 ? (bucket < 0 ? "adam" : bucket == 0 ? "adam_dec" : "adam_enc") : "shadow_refresh");
    launch_adam(h->cfg.compute_dtype, a, blocks, s);
    LAUNCH_OK(mode == 0 ? "adam" : "shadow_refresh");
}

// Clipping on: the partial sums of squares of the whole gradient buffer [0, P_int) (the cost slot stays out), ahead of the step's
// k_adam launch(es), which add them up.
void run_grad_sumsq(avae_handle* h, hipStream_t s) {
    ClipState* cs = h->clip_buf.as<ClipState>();
    if (!cs) throw Err("internal error: clipping is on without its device state");
    timed_launch(h, s, "grad_sumsq", [&] { launch_grad_sumsq(h->grad(), (long long)h->P_int, cs->partial, s); });
}

// Where the encoder's copy of a staged batch comes from when it is not the batch itself (include/avae.h, denoising training):
// the caller's explicit inputs (null, or null entries: none), else -- `corrupt`: the training calls -- the handle's corruption.
struct PrepIn { const float* const* in = nullptr; const int32_t* in_ld = nullptr; bool corrupt = false; };

// The staging kernel's arguments (k_prep).  Three fillers shared by the batch form (every modality + eps, the training / eval
// calls) and the single form (one source per launch, the forward-only calls): the generator's key, one segment, the eps block.
PrepArgs new_prep(const avae_handle* h, unsigned long long salt, int row0 = 0) {
    PrepArgs a;
    std::memset(&a, 0, sizeof(a));
    a.row_offset = h->cfg.row_offset + row0; a.seed = h->cfg.seed; a.st = h->state(); a.stream_salt = salt;
    return a;
}

// rows x cols fp32 of src -> compute-dtype rows of dst (+ their exact fp32 copy in dst32); returns the segment's tiles
int fill_prep_seg(const avae_handle* h, PrepSeg& g, const float* src, int src_ld, int rows, int cols, const Act& dst, float* dst32,
                  int ld32, int tile_base) {
    g.src = src; g.src_ld = src_ld; g.rows = rows; g.cols = cols;
    g.dst32 = dst32; g.ld32 = ld32;
    g.dstc = h->at<void>(dst.rm); g.ldc = dst.ld;
    g.tiles_r = (rows + 63) / 64; g.tiles_c = (cols + 63) / 64; g.tile_base = tile_base;
    return g.tiles_r * g.tiles_c;
}

// eps of `rows` rows into the eps buffer: the caller's, or (null) drawn by the generator
void fill_prep_eps(const avae_handle* h, PrepArgs& a, const float* eps, int rows) {
    a.eps_src = eps; a.eps_dst = h->at<float>(h->off_eps); a.eps_rows = rows; a.nz = h->nz; a.eps_ld = h->ld_eps;
    a.eps_blocks = (rows * ((h->nz + 3) / 4) + kThreads - 1) / kThreads;
}

// stages the caller's batch (and eps) into the internal compute-dtype buffers
PrepArgs make_prep_batch(avae_handle* h, const float* const* x, const int32_t* x_ld, const float* eps, int rows,
                         unsigned long long salt, int n_steps = 1, const uint8_t* present = nullptr, const PrepIn& pin = PrepIn()) {
    PrepArgs a = new_prep(h, salt);
    int base = 0;
    for (int m = 0; m < h->M; ++m) {
        const Mod& md = h->mods[m];
        PrepSeg& g = a.seg[m];
        base += fill_prep_seg(h, g, x[m], (x_ld && x_ld[m] > 0) ? x_ld[m] : md.n_in, rows, md.n_in, md.X0, h->at<float>(md.X32), md.ld32, base);
        if (pin.in && pin.in[m]) {
            g.src_in = pin.in[m]; g.in_ld = (pin.in_ld && pin.in_ld[m] > 0) ? pin.in_ld[m] : md.n_in;
            a.noisy = 1;
        } else if (pin.corrupt && (h->drop_thr[m] != 0u || h->corr.noise_std[m] > 0.0f)) {
            g.drop_thr = h->drop_thr[m]; g.drop_value = h->corr.drop_value[m]; g.noise_std = h->corr.noise_std[m];
            a.noisy = 1;
        }
    }
    a.n_seg = h->M; a.total_tiles = base;
    fill_prep_eps(h, a, eps, rows);
    a.n_steps = n_steps; a.blocks_per_step = a.total_tiles + a.eps_blocks; a.set_stride = (long long)h->stage_bytes;
    if (present) { a.pres_src = present; a.pres_dst = h->pres_buf.as<unsigned char>(); a.pres_ld = h->M; }      // masked staging (set j at j * rows * M)
    if (h->sched_on && salt == kTrainSalt) a.sched = h->sched_buf.as<SchedState>();      // training staging: this submission's schedule entries
    return a;
}

void run_prep_batch(avae_handle* h, const float* const* x, const int32_t* x_ld, const float* eps, int rows,
                    unsigned long long salt, hipStream_t s, const uint8_t* present = nullptr, int n_steps = 1, const PrepIn& pin = PrepIn()) {
    const PrepArgs a = make_prep_batch(h, x, x_ld, eps, rows, salt, n_steps, present, pin);
    timed_launch(h, s, "prep", [&] { launch_prep(h->cfg.compute_dtype, a, s); });
}

// One source staged by a launch of its own (the forward-only calls): `rows` rows of `cols` floats at src -> dst.  The rest is
// optional and named.
struct PrepOne {
    const float* src; int src_ld, rows, cols;
    const Act& dst;
    int row0;                                  // the rows' index in the whole input (keys the generator: row0 + row)
    PrepOne(const float* src_, int src_ld_, int rows_, int cols_, const Act& dst_, int row0_ = 0)
        : src(src_), src_ld(src_ld_), rows(rows_), cols(cols_), dst(dst_), row0(row0_) {}
    float* dst32 = nullptr; int ld32 = 0;      // an exact fp32 copy of the rows
    bool eps = false;                          // also stage eps for these rows: eps_src, or (null) a draw keyed by salt and row
    const float* eps_src = nullptr;
    unsigned long long salt = 0;
    PrepOne& with_eps(const float* e, unsigned long long salt_ = 0) { eps = true; eps_src = e; salt = salt_; return *this; }
    // masked staging: this modality's column of the caller's [rows][pres_ld] presence bytes and of their staged copy, so that the
    // segment's index 0 addresses it; a null src is then a modality absent on every row, staged as zeros
    const unsigned char* pres_src = nullptr; unsigned char* pres_dst = nullptr; int pres_ld = 0;
};

void run_prep_single(avae_handle* h, const PrepOne& p, hipStream_t s) {
    PrepArgs a = new_prep(h, p.salt, p.row0);
    if (p.pres_src) { a.pres_src = p.pres_src; a.pres_dst = p.pres_dst; a.pres_ld = p.pres_ld; }
    if (p.src || p.pres_src) {
        a.n_seg = 1;
        a.total_tiles = fill_prep_seg(h, a.seg[0], p.src, p.src_ld, p.rows, p.cols, p.dst, p.dst32, p.ld32, 0);
    }
    if (p.eps) fill_prep_eps(h, a, p.eps_src, p.rows);
    launch_prep(h->cfg.compute_dtype, a, s);
    LAUNCH_OK("prep");
}

// Captures body (timing off); with_prep: a step graph whose one root node is the input-staging kernel -- its template and that node
// are kept for patch_prep.
StepGraph capture(avae_handle* h, const std::function<void(hipStream_t)>& body, bool with_prep = false) {
    StepGraph sg;
    const bool tsave = h->timing;
    h->timing = false;
    HIP_OK(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
    try { body(h->cap_stream); }
    catch (...) { (void)hipStreamEndCapture(h->cap_stream, &sg.graph); sg.release(); h->timing = tsave; throw; }
    h->timing = tsave;
    HIP_OK(hipStreamEndCapture(h->cap_stream, &sg.graph));
    try {
        if (with_prep) {
            size_t n_root = 0;
            HIP_OK(hipGraphGetRootNodes(sg.graph, nullptr, &n_root));
            if (n_root != 1) throw Err("internal error: the captured step is not a chain");
            HIP_OK(hipGraphGetRootNodes(sg.graph, &sg.prep, &n_root));
            hipGraphNodeType ty;
            HIP_OK(hipGraphNodeGetType(sg.prep, &ty));
            if (ty != hipGraphNodeTypeKernel) throw Err("internal error: the captured step does not start with the staging kernel");
        }
        HIP_OK(hipGraphInstantiate(&sg.exec, sg.graph, nullptr, nullptr, 0));
        if (!with_prep) { HIP_OK(hipGraphDestroy(sg.graph)); sg.graph = nullptr; }
    } catch (...) { sg.release(); throw; }
    return sg;
}

// Points a step graph's staging node at the caller's batch (or run of n_steps consecutive batches).
void patch_prep(avae_handle* h, const StepGraph& sg, const float* const* x, const int32_t* x_ld, const float* eps,
                int n_steps, const uint8_t* present, const PrepIn& pin) {
    PrepArgs a = make_prep_batch(h, x, x_ld, eps, h->B, kTrainSalt, n_steps, present, pin);
    void* kp[1] = {&a};
    hipKernelNodeParams np;
    std::memset(&np, 0, sizeof(np));
    np.func = const_cast<void*>(prep_kernel(h->cfg.compute_dtype, present != nullptr, a.noisy != 0, a.sched != nullptr));
    np.gridDim = dim3((a.total_tiles + a.eps_blocks) * n_steps); np.blockDim = dim3(kThreads);
    np.sharedMemBytes = 0; np.kernelParams = kp; np.extra = nullptr;
    HIP_OK(hipGraphExecKernelNodeSetParams(sg.exec, sg.prep, &np));
}

void fill_ones(avae_handle* h, const Act& a, hipStream_t s) {
    if (!a.ones) return;
    const unsigned bits = h->es == 2 ? 0x3F80u : 0x3F800000u;
    launch_fill(h->at<void>(a.rm), h->es, bits, a.width, a.ld, h->B, s);             // column `width`, rows < B
    LAUNCH_OK("fill");
}

// One step on staging set j (forward launches `fwd`: a plan's): forward, backward, then the weight gradients with Adam in their
// epilogue, or followed by k_adam; with clipping on always weight gradients -> k_grad_sumsq -> k_adam, with averaging on always
// weight gradients -> k_adam (the fused epilogue knows neither).
// more: step j + 1 of the same graph follows (its first launch's descriptors are warmed by this step's last launch).  That step
// overwrites this one's gradient before any host code runs, and in the fused plan nothing on the device reads the gradient, so the
// descriptor wgrad+adam launches of such a step do not store it (k_small_tn_nograd); the last step of every graph and every eager
// step do, and AVAE_KEEP_GRADS=1 makes every step.  Returns whether this step's gradient is in the gradient buffer afterwards.
bool step_body(avae_handle* h, const std::vector<Launch>& fwd, hipStream_t s, int j, int stamp_base = -1, bool more = false) {
    auto sb = [&](size_t k) { return stamp_base < 0 ? -1 : stamp_base + (int)k; };
    auto first_of = [](const std::vector<Launch>& ls) { return ls.empty() ? nullptr : &ls[0]; };
    const bool fused = !h->wgrad_adam.empty() && !h->clip_on && !h->ema_on;
    run_set(h, fwd, 0, fwd.size(), j, s, stamp_base, true, first_of(h->bwd), j);
    const bool plain = &fwd == &h->plain.fwd;      // (the masked twin's head and loss launches stay by-value; the backward launches are shared)
    run_set(h, h->bwd, 0, h->bwd.size(), j, s, sb(fwd.size()), true, fused ? first_of(h->wgrad_adam) : nullptr, j, plain);
    if (fused) {       // the optimiser rides in the weight-gradient launch
        bool keep = !more || h->sw.keep_grads;
        for (const Launch& L : h->wgrad_adam) keep = keep || !(L.tn && L.cfg == kLeanTnAdam && L.desc_n);     // a by-value launch always stores
        run_set(h, h->wgrad_adam, 0, h->wgrad_adam.size(), j, s, sb(fwd.size() + h->bwd.size()), true, more ? first_of(fwd) : nullptr, j + 1, true, keep);
        return keep;
    }
    run_set(h, h->wgrad, 0, h->wgrad.size(), j, s, sb(fwd.size() + h->bwd.size()), true);
    if (h->clip_on) run_grad_sumsq(h, s);
    run_adam(h, 0, s);
    return true;
}

// The training graphs of plan p (what avae_set_grad_clip / avae_set_ema capture again when the step's tail changes; eval holds no optimiser).
// `present` non-null: the masked plan (masked staging; the placeholder is patched per replay like the inputs).  On failure p keeps
// none of them.
void capture_steps(avae_handle* h, StepPlan& p, const uint8_t* present) {
    std::vector<const float*> x0(h->M, h->at<float>(h->mods[0].X32));    // placeholders, patched per step
    try {
        std::vector<unsigned char> keep;
        p.full = capture(h, [&](hipStream_t cs) {
            run_prep_batch(h, x0.data(), nullptr, nullptr, h->B, kTrainSalt, cs, present);
            keep.push_back(step_body(h, p.fwd, cs, 0, 0));
        }, true);
        p.full.grad_keep = keep;
        // avae_train_steps: kMultiSizes[gi] whole steps per replay (a replay boundary costs ~5 us of idle GPU on this stack), their
        // batches staged by ONE launch into as many staging sets; step j's launches read set j
        for (int gi = 0; gi < 2; ++gi) {
            keep.clear();
            p.multi[gi] = capture(h, [&](hipStream_t cs) {
                run_prep_batch(h, x0.data(), nullptr, nullptr, h->B, kTrainSalt, cs, present, kMultiSizes[gi]);
                for (int j = 0; j < kMultiSizes[gi]; ++j) keep.push_back(step_body(h, p.fwd, cs, j, -1, j + 1 < kMultiSizes[gi]));
            }, true);
            p.multi[gi].grad_keep = keep;
        }
    } catch (...) { p.full.release(); p.multi[0].release(); p.multi[1].release(); throw; }
}

// All graphs of plan p.  On failure p keeps no graph.
void capture_plan(avae_handle* h, StepPlan& p, const uint8_t* present) {
    try {
        capture_steps(h, p, present);
        p.eval = capture(h, [&](hipStream_t cs) { run_launches(h, p.fwd, cs); run_launch(h, h->cost_only, cs, nullptr, -1); });
    } catch (...) { p.release(); throw; }
}

void init_device(avae_handle* h) {
    hipStream_t s = h->cap_stream;
    HIP_OK(hipMemsetAsync(h->ws, 0, h->ws_bytes, s));
    for (const Mod& md : h->mods) {
        for (int j = 0; j < kMultiSteps; ++j) {       // every staging set carries its own constant-1 column
            Act x = md.X0;
            x.rm += (size_t)j * h->stage_bytes;
            fill_ones(h, x, s);
        }
        for (const Act& a : md.E) fill_ones(h, a, s);
        fill_ones(h, md.Z, s);
        for (const Act& a : md.D) fill_ones(h, a, s);
        if (md.conv && md.cdec[3].dense_map) fill_ones(h, md.cdec[3].Y, s);      // the dense 28x28 map feeds the output layer: its bias column
    }
    build_training_plan(h);
    build_descriptors(h, s);
    HIP_OK(hipMemcpyAsync(h->at<void>(h->off_adam), h->adam_items.data(), h->adam_items.size() * sizeof(AdamItem), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(h->at<void>(h->off_adam_b), h->adam_items_b.data(), h->adam_items_b.size() * sizeof(AdamItem), hipMemcpyHostToDevice, s));
    {   // the two constant chunks an implicit patch matrix reads instead of an invalid tap / as its bias column, and the descriptors
        static const unsigned char c32_bf16[32] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x80, 0x3F};         // bf16 1.0 = 0x3F80, little endian
        static const unsigned char c32_f32[32] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x80, 0x3F};      // fp32 1.0 = 0x3F800000
        HIP_OK(hipMemcpyAsync(h->at<void>(h->off_consts), h->es == 2 ? c32_bf16 : c32_f32, 32, hipMemcpyHostToDevice, s));
        if (!h->conv_tab.empty()) {
            const unsigned char* lo = h->ws + h->stage_lo;
            for (const ConvA& c : h->conv_tab)
                if (reinterpret_cast<const unsigned char*>(c.src) >= lo && reinterpret_cast<const unsigned char*>(c.src) < lo + h->stage_bytes * kMultiSteps)
                    throw Err("internal error: an implicit patch matrix on a staged input (not relocatable per step)");
            HIP_OK(hipMemcpyAsync(h->at<void>(h->off_conv_tab), h->conv_tab.data(), h->conv_tab.size() * sizeof(ConvA), hipMemcpyHostToDevice, s));
        }
    }
    size_t off = h->off_inf;
    h->inf_enc.assign(h->M, avae_handle::Inf());
    h->inf_dec.assign(h->M, avae_handle::Inf());
    for (int m = 0; m < h->M; ++m) {
        h->inf_enc[m].dev_off = off; off += ((size_t)h->mods[m].L + 1) * sizeof(WorkItem);
        h->inf_dec[m].dev_off = off; off += ((size_t)h->mods[m].L + 1) * sizeof(WorkItem);
    }
    HIP_OK(hipStreamSynchronize(s));
    if (h->cfg.use_graph) capture_plan(h, h->plain, nullptr);
}

void comm_check_error(avae_handle* h);

void fetch_cost(avae_handle* h, float* cost_host, bool from_state, hipStream_t s) {
    if (!cost_host) return;
    const void* src = from_state ? (const void*)&h->state()->last_cost : (const void*)(h->grad() + h->P_int);
    HIP_OK(hipMemcpyAsync(cost_host, src, sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    comm_check_error(h);
}

void copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows, hipStream_t s) {
    HIP_OK(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToDevice, s));
}

// start of every stream-taking call (under the handle's mutex)
hipStream_t on_stream(avae_handle* h, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (h->has_last_stream && s != h->last_stream) {
        if (!h->ev_switch) HIP_OK(hipEventCreateWithFlags(&h->ev_switch, hipEventDisableTiming));
        if (hipEventRecord(h->ev_switch, h->last_stream) == hipSuccess) HIP_OK(hipStreamWaitEvent(s, h->ev_switch, 0));
        else (void)hipGetLastError();          // the previous stream no longer exists: its work is done
    }
    h->last_stream = s; h->has_last_stream = true;
    return s;
}

// avae_set_schedule / avae_schedule_value: the ranges of include/avae.h; `who` names the call and the schedule, the message the field.
void check_schedule(const avae_schedule& c, const std::string& who) {
    auto fail = [&](const std::string& what) { throw Err(who + ": " + what); };
    if (c.kind == AVAE_SCHED_NONE) return;
    if (c.kind == AVAE_SCHED_PIECEWISE) {
        if (c.n_knots < 1 || c.n_knots > AVAE_SCHED_MAX_KNOTS)
            fail("n_knots = " + std::to_string(c.n_knots) + " must be in [1, " + std::to_string(AVAE_SCHED_MAX_KNOTS) + "]");
        if (c.period < 0) fail("period = " + std::to_string((long long)c.period) + " must be >= 0");
        for (int i = 0; i < c.n_knots; ++i) {
            if (i == 0 ? c.knot_step[0] < 0 : c.knot_step[i] <= c.knot_step[i - 1])
                fail("knot_step[" + std::to_string(i) + "] = " + std::to_string((long long)c.knot_step[i]) +
                     (i == 0 ? " must be >= 0" : " must be above knot_step[" + std::to_string(i - 1) + "] (strictly increasing)"));
            if (!(c.knot_value[i] >= 0.0f) || std::isinf(c.knot_value[i]))
                fail("knot_value[" + std::to_string(i) + "] must be finite and >= 0");
        }
        if (c.period > 0 && c.knot_step[c.n_knots - 1] >= c.period)
            fail("knot_step[" + std::to_string(c.n_knots - 1) + "] = " + std::to_string((long long)c.knot_step[c.n_knots - 1]) +
                 " must be below period = " + std::to_string((long long)c.period));
        return;
    }
    if (c.kind == AVAE_SCHED_EXP) {
        if (!(c.decay_rate > 0.0f) || std::isinf(c.decay_rate)) fail("decay_rate must be finite and > 0");
        if (c.decay_steps <= 0) fail("decay_steps = " + std::to_string((long long)c.decay_steps) + " must be > 0");
        if (c.staircase != 0 && c.staircase != 1) fail("staircase must be 0 or 1");
        return;
    }
    fail("kind = " + std::to_string(c.kind) + " is none of AVAE_SCHED_NONE, AVAE_SCHED_PIECEWISE, AVAE_SCHED_EXP");
}

// A checked schedule with the fields its kind does not read zeroed (what the device keeps).
avae_schedule canonical_schedule(const avae_schedule& c) {
    avae_schedule o;
    std::memset(&o, 0, sizeof(o));
    o.kind = c.kind;
    if (c.kind == AVAE_SCHED_PIECEWISE) {
        o.n_knots = c.n_knots; o.period = c.period;
        for (int i = 0; i < c.n_knots; ++i) { o.knot_step[i] = c.knot_step[i]; o.knot_value[i] = c.knot_value[i]; }
    } else if (c.kind == AVAE_SCHED_EXP) {
        o.decay_rate = c.decay_rate; o.staircase = c.staircase; o.decay_steps = c.decay_steps;
    }
    return o;
}

template <typename F> int guarded(avae_handle* h, F&& f) {
    if (!h) return 1;
    std::lock_guard<std::mutex> lk(h->mu);
    try {
        DeviceGuard dg(h->cfg.device);
        f();
        return 0;
    } catch (const std::exception& e) {
        h->err = e.what();
        return 2;
    }
}

void master_to_host(avae_handle* h, size_t off, std::vector<float>& host) {
    host.resize(h->P_int);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(host.data(), h->at<void>(off), h->P_int * 4, hipMemcpyDeviceToHost));
}
void host_to_master(avae_handle* h, size_t off, const std::vector<float>& host) {
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(h->at<void>(off), host.data(), h->P_int * 4, hipMemcpyHostToDevice));
}

// ----------------------------------------------------------------------------- RCCL (loaded at run time)
// The process usually has an RCCL already (PyTorch-ROCm bundles one): that copy is used when present, the system's otherwise.
// Only the five entry points the gradient all-reduce needs are bound; no RCCL header is needed at build time.
struct Rccl {
    struct Id { char b[128]; };                 // ncclUniqueId (passed by value)
    typedef int (*get_id_t)(void*);
    typedef int (*init_rank_t)(void**, int, Id, int);
    typedef int (*all_reduce_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
    typedef int (*destroy_t)(void*);
    typedef const char* (*err_t)(int);
    typedef int (*group_t)();
    void* lib = nullptr;
    get_id_t get_id = nullptr; init_rank_t init_rank = nullptr; all_reduce_t all_reduce = nullptr; destroy_t destroy = nullptr;
    err_t err_str = nullptr; group_t group_start = nullptr, group_end = nullptr;
    static Rccl& get() {
        static Rccl r;
        static std::once_flag once;
        std::call_once(once, [] {
            const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
            for (const char* n : names) if ((r.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;       // the copy already in the process
            for (const char* n : names) { if (r.lib) break; r.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL); }
            if (!r.lib) return;
            r.get_id = (get_id_t)dlsym(r.lib, "ncclGetUniqueId"); r.init_rank = (init_rank_t)dlsym(r.lib, "ncclCommInitRank");
            r.all_reduce = (all_reduce_t)dlsym(r.lib, "ncclAllReduce"); r.destroy = (destroy_t)dlsym(r.lib, "ncclCommDestroy");
            r.err_str = (err_t)dlsym(r.lib, "ncclGetErrorString");
            r.group_start = (group_t)dlsym(r.lib, "ncclGroupStart"); r.group_end = (group_t)dlsym(r.lib, "ncclGroupEnd");
        });
        if (!r.lib || !r.get_id || !r.init_rank || !r.all_reduce || !r.destroy || !r.group_start || !r.group_end)
            throw Err("RCCL is not available (librccl.so could not be loaded): the library-owned gradient all-reduce needs it");
        return r;
    }
};
#define NCCL_OK(expr)                                                                            \
    do {                                                                                         \
        int r_ = (expr);                                                                         \
        if (r_ != 0) throw Err(std::string(#expr) + ": " + (Rccl::get().err_str ? Rccl::get().err_str(r_) : "RCCL error") + " (" + std::to_string(r_) + ")"); \
    } while (0)
constexpr int kNcclFloat32 = 7, kNcclSum = 0;        // rccl.h: ncclFloat32, ncclSum (ncclBfloat16 = 9)

constexpr int kNcclBfloat16 = 9;
constexpr uint32_t kIpcMagic = 0x41564950u;      // "AVIP"
struct IpcHandleBytes {                          // what avae_comm_ipc_handle hands out (AVAE_IPC_HANDLE_BYTES)
    hipIpcMemHandle_t mem;                       // 64 bytes
    uint64_t bytes, raw_ptr, layout;             // block size; the exporter's own pointer (same-process attach); layout check word
    int32_t rank, world, pid;
    uint32_t magic;
};
static_assert(sizeof(IpcHandleBytes) <= AVAE_IPC_HANDLE_BYTES, "IPC handle bytes");
static_assert(kMaxWorld == AVAE_MAX_WORLD, "world size limit");

void comm_streams(avae_handle* h) {
    int lo = 0, hi = 0;                          // the collective's kernels should start the moment their gradients exist
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (h->sw.comm_no_prio) hi = 0;     // (A/B)
    HIP_OK(hipStreamCreateWithPriority(&h->comm_stream, hipStreamNonBlocking, hi));
    for (int b = 0; b < 2; ++b) {
        HIP_OK(hipEventCreateWithFlags(&h->ev_grad[b], hipEventDisableTiming));
        HIP_OK(hipEventCreateWithFlags(&h->ev_red[b], hipEventDisableTiming));
    }
    h->comm_world = h->cfg.world_size; h->comm_rank = h->cfg.rank;
    h->comm_on = true;
}

void comm_init_rccl(avae_handle* h) {
    Rccl& R = Rccl::get();
    Rccl::Id id;
    std::memcpy(id.b, h->cfg.nccl_id, 128);
    {   // RCCL prints a version banner on stdout when its first communicator comes up; the host's stdout may be a protocol
        // (bench.py: one JSON line): send it to stderr
        std::fflush(stdout);
        const int saved = dup(1);
        if (saved >= 0) (void)dup2(2, 1);
        const int rc = R.init_rank(&h->comm, h->cfg.world_size, id, h->cfg.rank);
        std::fflush(stdout);
        if (saved >= 0) { (void)dup2(saved, 1); (void)close(saved); }
        NCCL_OK(rc);
    }
    comm_streams(h);
}

// Exchange block of the one-shot all-reduce: [flag1 | flag2 | costs | seq | err | slots (one per source rank) | result area]
void comm_init_ipc(avae_handle* h) {
    const int N = h->cfg.world_size;
    IpcArgs& a = h->ipc_args;
    std::memset(&a, 0, sizeof(a));
    const int blocks = h->sw.ipc_blocks;
    if (blocks < 1 || blocks > 1024) throw Err("AVAE_IPC_BLOCKS out of range");
    const bool bf = h->cfg.wire_dtype == AVAE_BF16;
    const size_t gb = bf ? 16 : 32, G = h->P_int / 8, S = (G + N - 1) / N;        // (P_int is a multiple of 32 floats)
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = rup(off + bytes, 256); return o; };
    a.off_flag1 = (long long)take((size_t)blocks * kMaxWorld * 4);
    a.off_flag2 = (long long)take((size_t)blocks * kMaxWorld * 4);
    a.off_cost = (long long)take(kMaxWorld * 4);
    a.off_seq = (long long)take((size_t)blocks * 4);
    a.off_err = (long long)take(4);
    a.slot_stride = (long long)rup(S * gb, 256);
    a.off_slots = (long long)take((size_t)N * a.slot_stride);
    a.off_res = (long long)take(G * gb);
    h->ipc_bytes = off;
    a.g = h->grad(); a.world = N; a.rank = h->cfg.rank; a.wire_bf16 = bf ? 1 : 0; a.blocks = blocks;
    a.timeout_ticks = (unsigned long long)(h->sw.ipc_timeout_ms * 1e5);                            // 100 MHz wall clock
    // uncached: neither this device's L2s nor a peer's keep lines of it (RCCL allocates its own buffers the same way)
    HIP_OK(hipExtMallocWithFlags(reinterpret_cast<void**>(&h->ipc_block), h->ipc_bytes, hipDeviceMallocUncached));
    HIP_OK(hipMemset(h->ipc_block, 0, h->ipc_bytes));
    HIP_OK(hipDeviceSynchronize());
    a.peer[h->cfg.rank] = h->ipc_block; h->ipc_peer[h->cfg.rank] = h->ipc_block;
    comm_streams(h);
    h->ipc_attached = N == 1;
}

void comm_init(avae_handle* h) {
    if (h->cfg.world_size < 1 || h->cfg.world_size > kMaxWorld || h->cfg.rank < 0 || h->cfg.rank >= h->cfg.world_size)
        throw Err("use_comm: world_size must be in [1," + std::to_string(kMaxWorld) + "] and rank in [0, world_size)");
    if (h->cfg.use_comm == AVAE_COMM_RCCL) comm_init_rccl(h);
    else if (h->cfg.use_comm == AVAE_COMM_IPC) comm_init_ipc(h);
    else throw Err("use_comm must be AVAE_COMM_NONE, AVAE_COMM_RCCL or AVAE_COMM_IPC");
}

uint64_t ipc_layout_word(const avae_handle* h) {
    return (uint64_t)h->P_int * 1315423911ull ^ ((uint64_t)h->ipc_args.blocks << 48) ^ ((uint64_t)h->ipc_args.wire_bf16 << 40) ^ (uint64_t)h->ipc_bytes;
}

void comm_check_error(avae_handle* h) {       // after a synchronise: did a bounded wait of the IPC all-reduce give up?
    if (!h->ipc_block) return;
    unsigned e = 0;
    HIP_OK(hipMemcpy(&e, h->ipc_block + h->ipc_args.off_err, 4, hipMemcpyDeviceToHost));
    if (e) {
        std::string who;
        for (int r = 0; r < kMaxWorld; ++r) if (e & (1u << (8 + r))) who += " " + std::to_string(r);
        throw Err("IPC all-reduce: timed out waiting for rank(s)" + who + " (phase mask " + std::to_string(e & 0xFFu) +
                  "): a peer stopped, or the ranks did not make the same sequence of training calls");
    }
}

// ranges of bucket b, from the memory plan alone (so that avae_dp_plan needs no device): ONE contiguous range per bucket
void dp_ranges(const avae_handle* h, int* n_buckets, std::vector<avae_handle::Range> (&out)[2]) {
    bool any_conv = false;
    for (const Mod& md : h->mods) any_conv = any_conv || md.conv;
    out[0].clear(); out[1].clear();
    // comm_buckets = 1: north_star's literal design, a single all-reduce of the whole buffer (gradient + cost)
    if (any_conv || h->cfg.comm_buckets == 1) { *n_buckets = 1; out[0].push_back({0, h->P_int + 1}); return; }
    *n_buckets = 2;
    out[1].push_back({0, h->P_enc});                               // encoder sides of every modality
    out[0].push_back({h->P_enc, h->P_int + 1 - h->P_enc});         // decoder sides + the cost slot (element P_int)
}

// forward + the backward part of bucket b + its weight gradients, on staging set j
void dp_segment(avae_handle* h, int j, int bucket, hipStream_t s, bool direct = false) {
    if (bucket < 0 || bucket >= h->n_buckets) throw Err("data-parallel bucket out of range");
    if (j < 0 || j >= kMultiSteps) throw Err("staging set out of range");
    auto body = [&](hipStream_t cs) {
        auto run = [&](const std::vector<Launch>& ls, size_t lo, size_t hi) { run_set(h, ls, lo, hi, j, cs, -1, true); };
        if (h->n_buckets == 1) { run(h->plain.fwd, 0, h->plain.fwd.size()); run(h->bwd, 0, h->bwd.size()); run(h->wgrad, 0, h->wgrad.size()); return; }
        if (bucket == 0) { run(h->plain.fwd, 0, h->plain.fwd.size()); run(h->bwd, 0, (size_t)h->bwd_split); run(h->wgrad_b[0], 0, h->wgrad_b[0].size()); }
        else { run(h->bwd, (size_t)h->bwd_split, h->bwd.size()); run(h->wgrad_b[1], 0, h->wgrad_b[1].size()); }
    };
    if (h->cfg.use_graph && !h->timing && !direct) {
        if (h->g_dp[bucket].empty()) h->g_dp[bucket].resize(kMultiSteps);
        if (!h->g_dp[bucket][j].exec) h->g_dp[bucket][j] = capture(h, body);
        HIP_OK(hipGraphLaunch(h->g_dp[bucket][j].exec, s));
    } else {
        body(s);
    }
}

// SUM-all-reduce of bucket b's range of the gradient buffer on the comm stream (either backend)
void dp_allreduce(avae_handle* h, int b, hipStream_t cs) {
    const avae_handle::Range& r = h->ranges_b[b][0];
    float* g = h->grad();
    const bool has_cost = r.off + r.count == h->P_int + 1;
    const size_t n = has_cost ? r.count - 1 : r.count;               // the gradient part: a multiple of 32 floats
    Timed t(h, cs, h->n_buckets == 1 ? "allreduce" : b == 0 ? "allreduce_dec" : "allreduce_enc");
    t_launch_events = LaunchEvents{nullptr, nullptr};               // (several enqueues: bracket them with plain records instead)
    if (t.on) (void)hipEventRecord(t.a, cs);
    if (h->cfg.use_comm == AVAE_COMM_IPC) {
        if (!h->ipc_attached) throw Err("AVAE_COMM_IPC: avae_comm_ipc_attach has not been called on this replica");
        IpcArgs a = h->ipc_args;
        a.off = (long long)r.off; a.granules = (long long)(n / 8); a.cost_idx = has_cost ? (long long)h->P_int : -1;
        launch_ipc_allreduce(a, cs);
        LAUNCH_OK("ipc_allreduce");
    } else {
        Rccl& R = Rccl::get();
        if (h->cfg.wire_dtype == AVAE_BF16) {                      // bf16 on the wire, the cost beside it in fp32
            unsigned short* wire = h->at<unsigned short>(h->off_wire) + r.off;
            launch_wire_pack(g + r.off, wire, (long long)n, cs); LAUNCH_OK("wire_pack");
            NCCL_OK(R.group_start());
            NCCL_OK(R.all_reduce(wire, wire, n, kNcclBfloat16, kNcclSum, h->comm, cs));
            if (has_cost) NCCL_OK(R.all_reduce(g + h->P_int, g + h->P_int, 1, kNcclFloat32, kNcclSum, h->comm, cs));
            NCCL_OK(R.group_end());
            launch_wire_unpack(g + r.off, wire, (long long)n, cs); LAUNCH_OK("wire_unpack");
        } else {
            NCCL_OK(R.all_reduce(g + r.off, g + r.off, r.count, kNcclFloat32, kNcclSum, h->comm, cs));
        }
    }
    if (t.on) (void)hipEventRecord(t.b, cs);
}

// one step of the library-owned data-parallel pipeline on staging set j (main stream s, collective on the comm stream)
void dp_step(avae_handle* h, int j, hipStream_t s, bool direct = false) {
    if (h->n_buckets == 1) {
        // one bucket: nothing to overlap, so everything stays on ONE stream -- a kernel on a second stream inside a captured graph
        // costs fork / join edges (measured, one rank: 0.0583 -> see DESIGN section 6; the two-bucket pipeline pays 35 us for them)
        dp_segment(h, j, 0, s, direct);
        dp_allreduce(h, 0, s);
        if (h->clip_on) run_grad_sumsq(h, s);       // the norm is that of the REDUCED gradient: every rank forms the same c
        run_adam(h, 0, s, -1);
        return;
    }
    for (int b = 0; b < h->n_buckets; ++b) {
        dp_segment(h, j, b, s, direct);
        HIP_OK(hipEventRecord(h->ev_grad[b], s));
        HIP_OK(hipStreamWaitEvent(h->comm_stream, h->ev_grad[b], 0));
        dp_allreduce(h, b, h->comm_stream);
        HIP_OK(hipEventRecord(h->ev_red[b], h->comm_stream));
    }
    if (h->clip_on) {       // the norm needs BOTH reduced buckets before either is applied
        for (int b = 0; b < h->n_buckets; ++b) HIP_OK(hipStreamWaitEvent(s, h->ev_red[b], 0));
        run_grad_sumsq(h, s);
        for (int b = 0; b < h->n_buckets; ++b) run_adam(h, 0, s, b);
        return;
    }
    for (int b = 0; b < h->n_buckets; ++b) {
        HIP_OK(hipStreamWaitEvent(s, h->ev_red[b], 0));
        run_adam(h, 0, s, h->n_buckets == 1 ? -1 : b);
    }
}

// ----------------------------------------------------------------------------- serving
// generate() of every (MLP) modality in one submission per call (the reference's CEM / GUI callers decode
// 10-50 times per iteration, baxter_vae_assoc_writer.py:141-147,259-304, vae_assoc_model_viewer.py:107-113).
avae_handle::Serve& serve_plan(avae_handle* h, int bucket) {
    for (avae_handle::Serve& sv : h->serve) if (sv.bucket == bucket) return sv;
    h->serve.emplace_back();
    avae_handle::Serve& sv = h->serve.back();
    sv.bucket = bucket;
    Builder bd(h, sv.items, bucket, false);
    Groups group{h, sv.items};
    int Lmax = 0;
    for (const Mod& md : h->mods) Lmax = std::max(Lmax, md.L);
    // The decoder's first layer (K = n_z + 1) rides in the per-call staging launch when that fits its tail product (K_SERVE_Z: one K
    // tile of bf16, two of fp32, at most 1024 units, 32-row tiles); otherwise it is the graph's first launch behind k_serve.
    {
        const int first = (int)sv.items.size();
        bool fits = !h->sw.no_tail && bucket <= 4096;
        for (Mod& md : h->mods) {
            const WorkItem c = bd.fwd_hidden(md.Z, md.dec[0], md.D[0]);
            fits = fits && c.K <= (h->es == 2 ? 1 : 2) * h->KU && c.N <= 1024 && h->nz + 1 <= 64;
            WorkItem w = gemm_item(K_SERVE_Z, bucket, c.N, 0, nullptr, 0, nullptr, 0);
            w.nz = h->nz; w.partial = reinterpret_cast<float*>(h->at<ServeSlot>(h->off_slot));
            w.tail_mode = 1; w.tail_w = c.B; w.tail_ldw = c.ldb; w.tail_n = c.N; w.tail_out = c.out0; w.tail_ldo = c.ld0; w.tail_act = c.act;
            w.tail_kt = c.K / h->KU;
            sv.items.push_back(w);
        }
        if (fits) {
            sv.in_launch = finish_launch(h, sv.items, first, (int)sv.items.size() - first, "serve_in+serve_dec1", &group.slot);
            if (sv.in_launch.cfg != k32x64) fits = false;
        }
        if (fits && !h->sw.no_lean) {            // the same launch as a kernel of its own with a small argument block (k_serve_in)
            ServeInArgs& ia = sv.in_lean;
            std::memset(&ia, 0, sizeof(ia));
            ia.slot = h->at<ServeSlot>(h->off_slot); ia.n_mod = h->M; ia.nz = h->nz; ia.bucket = bucket; ia.tiles_m = (bucket + 31) / 32;
            int max_slices = 1;
            for (int m = 0; m < h->M; ++m) {
                const WorkItem& w = sv.items[first + m];
                ServeInMod& md = ia.mod[m];
                md.w = w.tail_w; md.out = w.tail_out; md.n = w.tail_n; md.ldw = w.tail_ldw; md.ldo = w.tail_ldo; md.kt = w.tail_kt; md.act = w.tail_act;
                md.slices = (w.tail_n + 63) / 64;
                max_slices = std::max(max_slices, md.slices);
            }
            sv.in_lean_grid = ia.tiles_m * max_slices;
            sv.lean_in = true;
        }
        if (!fits) sv.items.resize(first);
        sv.fused_in = fits;
    }
    for (int k = sv.fused_in ? 1 : 0; k < Lmax; ++k)
        group("serve_dec" + std::to_string(k + 1), sv.launches, [&] { for (Mod& md : h->mods) if (k < md.L) sv.items.push_back(bd.fwd_hidden(k == 0 ? md.Z : md.D[k - 1], md.dec[k], md.D[k])); });
    group("serve_out", sv.launches, [&] {
        for (int m = 0; m < h->M; ++m) {
            WorkItem w = bd.fwd_out(h->mods[m], m, false);
            w.aux2 = h->at<void>(h->off_slot); w.n_mod = m;       // K_FWD_OUT_STORE: rows and destination come from the slot
            sv.items.push_back(w);
        }
    });
    ServeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.slot = h->at<ServeSlot>(h->off_slot); a.n_mod = h->M; a.nz = h->nz; a.bucket = bucket;
    for (int m = 0; m < h->M; ++m) {
        const Mod& md = h->mods[m];
        a.Z[m] = h->at<void>(md.Z.rm); a.ldz[m] = md.Z.ld;
    }
    a.blocks_per_mod = std::max(1, std::min(8, (bucket * h->nz + kThreads - 1) / kThreads));
    sv.in = a;                                                   // the per-call staging launch (ahead of the graph)
    if (!(sv.fused_in && sv.lean_in))                            // serve_call replays a graph of the remaining launches
        sv.graph = capture(h, [&](hipStream_t cs) { run_launches(h, sv.launches, cs); }).exec;
    if (h->sw.plan_dump) {       // AVAE_PLAN_DUMP=1: the route and every launch of the plan, the staging launch first
        std::fprintf(stderr, "[avae] serve plan bucket=%d fused_in=%d lean_in=%d in_lean_grid=%d\n", bucket, sv.fused_in ? 1 : 0,
                     sv.lean_in ? 1 : 0, sv.in_lean_grid);
        if (sv.fused_in) dump_launch(sv.in_launch);
        for (const Launch& L : sv.launches) dump_launch(L);
        std::fflush(stderr);
    }
    return sv;
}

// One call through a serve plan: sl.rows rows of fp32 z (sl.z) decoded by every modality into sl.out.  With k_serve_in (which also
// runs the decoders' first layer): that launch and the plan's launches, eagerly.  Measured (tools/serve_latency.py, one box, 1 / 64
// rows, C ABI back to back, us per call): 14.6 / 15.6 eager against 19.1 / 19.9 for the staging launch + a graph replay of the rest,
// GPU-bound at three dependent kernels and a replay boundary of ~5 us.  Every other plan: its staging launch and one graph replay.
void serve_call(avae_handle* h, avae_handle::Serve& sv, const ServeSlot& sl, hipStream_t s) {
    if (sv.fused_in && sv.lean_in) {
        sv.in_lean.call = sl;
        launch_serve_in(h->cfg.compute_dtype, sv.in_lean, sv.in_lean_grid, s); LAUNCH_OK("serve_in+serve_dec1");
        run_launches(h, sv.launches, s);
        return;
    }
    if (sv.fused_in) {           // the staging launch also runs the decoder's first layer: its items carry the call by value
        Launch& L = sv.in_launch;
        for (int m = 0; m < h->M; ++m) {
            WorkItem& w = L.args.items[m];
            w.aux0 = sl.z; w.n_slots = sl.rows;
            w.out0 = sl.out[0]; w.out1 = sl.out[1]; w.out2 = sl.out[2]; w.aux1 = sl.out[3];
        }
        launch_grouped(h->cfg.compute_dtype, L.cfg, L.args, L.grid_x, L.grid_y, L.lds, h->state(), s, nullptr, 0); LAUNCH_OK("serve_in+serve_dec1");
    } else {
        launch_serve(h->cfg.compute_dtype, sv.in, sl, sv.in.blocks_per_mod * h->M, s); LAUNCH_OK("serve_in");
    }
    HIP_OK(hipGraphLaunch(sv.graph, s));
}

// The serve plan's row bucket for a call of n <= batch_size rows: the CEM / GUI callers' 1-64 rows, or a batch-sized chunk.
int serve_bucket(const avae_handle* h, int n) { return (n <= 64 && h->B > 64) ? 64 : h->B; }

// Conv decoders (and the diagnostic modes) decode modality by modality instead of through a serve plan.
bool decode_by_mod(const avae_handle* h) {
    for (const Mod& md : h->mods) if (md.conv) return true;
    return !h->cfg.use_graph || h->timing;
}

// A fresh eps per call, as each sess.run of the reference draws one (vae_assoc.py:90,388-391): the handle's 22-bit draw counter
// keys the generator; 0 when the caller gives eps.  Each caller places it in its own salt.
unsigned next_draw(avae_handle* h, const float* eps_dev) { return eps_dev ? 0u : (++h->draw_id) & 0x3FFFFFu; }

void run_inference(avae_handle* h, int m, bool enc, int rows, hipStream_t s) {
    build_inference(h, m, enc, rows);
    avae_handle::Inf& inf = enc ? h->inf_enc[m] : h->inf_dec[m];
    run_launches(h, inf.launches, s);          // items travel by value in the kernel arguments
}

// n decoded rows of modality m (out32, padded rows) -> dense caller rows
void copy_out32(avae_handle* h, int m, float* dst, int n, hipStream_t s) {
    const Mod& md = h->mods[m];
    copy_rows(dst, (size_t)md.n_in * 4, h->at<float>(md.out32), (size_t)md.ld32 * 4, (size_t)md.n_in * 4, n, s);
}

// rows rows of fp32 z (dense [rows][n_z]) through modality m's decoder into xhat (dense [rows][n_input]), batch_size at a time
void decode_rows(avae_handle* h, int m, const float* z, int rows, float* xhat, hipStream_t s) {
    const Mod& md = h->mods[m];
    for (int r0 = 0; r0 < rows; r0 += h->B) {
        const int n = std::min(h->B, rows - r0);
        run_prep_single(h, PrepOne(z + (size_t)r0 * h->nz, h->nz, n, h->nz, md.Z), s);
        run_inference(h, m, false, n, s);
        copy_out32(h, m, xhat + (size_t)r0 * md.n_in, n, s);
    }
}

// ----------------------------------------------------------------------------- forward-only row calls: the shared helpers
// avae_score / avae_loglik (+ _masked), avae_impute, avae_complete and avae_generate are put together from RowInputs, row_presence,
// stage_and_encode, DecodeAll and SampleBlocks below, PrepOne (run_prep_single's named arguments) and timed_launch above, and DevBuf
// (first-use scratch, one per entry point).  A new entry point starts from them.

// What a NULL x_dev[m] is: an error (avae_score, avae_loglik); a modality absent on every row (the _masked calls, avae_impute);
// an unobserved modality, of which at least one must be given (avae_complete).
enum class NullRows { Required, Absent, Unobserved };

// x_dev / x_ld of every modality (x_ld NULL: dense rows), resolved once per call; `what` prefixes the messages.  x_dev itself is
// not NULL: every caller checks that first, under its own name.
struct RowInputs {
    const float* x[kMaxMod] = {nullptr, nullptr, nullptr, nullptr};
    int ld[kMaxMod] = {0, 0, 0, 0};          // row stride; 0 for a NULL modality
    unsigned mods = 0;                       // bit m: x_dev[m] was given
    RowInputs(const avae_handle* h, const std::string& what, const float* const* x_dev, const int32_t* x_ld, NullRows rule) {
        for (int m = 0; m < h->M; ++m) {
            if (!x_dev[m]) {
                if (rule == NullRows::Required) throw Err(what + ": x_dev[" + std::to_string(m) + "] is NULL");
                continue;
            }
            x[m] = x_dev[m]; mods |= 1u << m;
            ld[m] = x_ld ? x_ld[m] : h->mods[m].n_in;
            if (ld[m] < h->mods[m].n_in)
                throw Err(what + ": x_ld[" + std::to_string(m) + "] = " + std::to_string(ld[m]) + " is below n_input = " + std::to_string(h->mods[m].n_in));
        }
        if (rule == NullRows::Unobserved && !mods) throw Err(what + ": every x_dev[m] is NULL (nothing is observed)");
    }
    const float* at(int m, int r0) const { return x[m] ? x[m] + (size_t)r0 * ld[m] : nullptr; }
};

// Masked calls: the caller's [rows][M] presence bytes and the chunk's staged copy [batch_size][M] that the kernels read (0 / 1,
// NULL sources folded in; DevBuf row_pres).  Both null for an unmasked call.
struct RowPresence {
    const uint8_t* src = nullptr;
    unsigned char* staged = nullptr;
    explicit operator bool() const { return src != nullptr; }
};

RowPresence row_presence(avae_handle* h, const uint8_t* present) {
    if (!present) return {};
    return {present, static_cast<unsigned char*>(h->row_pres.ensure((size_t)h->B * h->M))};
}

// eps staged together with the chunk's first modality (avae_score): the caller's rows (null: a draw) and the staging launches' salt
struct StageEps { const float* src; unsigned long long salt; };

// Rows [r0, r0 + n) of every modality -> its X0, with the chunk's presence bytes when masked, then its encoder.  A NULL modality
// of an unmasked call is skipped; of a masked call it is staged (zeros, absent on every row) and encoded only with encode_null.
void stage_and_encode(avae_handle* h, const RowInputs& in, const RowPresence& pres, int r0, int n, bool encode_null,
                      const StageEps* eps, hipStream_t s) {
    for (int m = 0; m < h->M; ++m) {
        if (!in.x[m] && !pres) continue;
        const Mod& md = h->mods[m];
        PrepOne p(in.at(m, r0), in.ld[m], n, md.n_in, md.X0, r0);
        if (eps && m == 0) p.with_eps(eps->src ? eps->src + (size_t)r0 * h->nz : nullptr);
        if (eps) p.salt = eps->salt;
        if (pres) { p.pres_src = pres.src + (size_t)r0 * h->M + m; p.pres_dst = pres.staged + m; p.pres_ld = h->M; }
        run_prep_single(h, p, s);
        if (in.x[m] || encode_null) run_inference(h, m, true, n, s);
    }
}

// "These z rows through every decoder."  The route is chosen once per call: by modality (conv decoders, use_graph = 0, timing),
// every decoder's own launches from its Z into its out32 (rows of ld32); else the serve route, the grouped launches of a serve
// plan in passes of at most batch_size rows, reading dense fp32 z and storing dense [rows][n_input] wherever the call points.
struct DecodeAll {
    avae_handle* h;
    bool by_mod;
    explicit DecodeAll(avae_handle* h_) : h(h_), by_mod(decode_by_mod(h_)) {}
    // Where a latent kernel (IwLatentArgs, ImputeFuseArgs) leaves z for run(): every decoder's Z, or the dense fp32 rows z32
    template <typename Args> void z_dest(Args& a, float* z32) const {
        if (!by_mod) { a.z32 = z32; return; }
        a.n_zdst = h->M;
        for (int m = 0; m < h->M; ++m) { a.Z[m] = h->at<void>(h->mods[m].Z.rm); a.ldz[m] = h->mods[m].Z.ld; }
    }
    // row stride of outputs left in decoder m's out32 (dst[m] null)
    int ld_out32(int m) const { return by_mod ? h->mods[m].ld32 : h->mods[m].n_in; }
    // nd rows.  z: dense fp32 [nd][n_z] -- read by the serve route; by modality only with stage_z (the caller's own z, any nd),
    // otherwise a latent kernel has filled the decoders' Z and nd <= batch_size.  dst (nullable, and per modality): dense
    // [nd][n_input] destinations; without one the rows stay in the decoder's out32.  dst_only: by modality, a decoder without a
    // destination does not run.
    void run(int nd, const float* z, bool stage_z, float* const* dst, bool dst_only, hipStream_t s) const {
        if (by_mod) {
            for (int m = 0; m < h->M; ++m) {
                float* out = dst ? dst[m] : nullptr;
                if (dst_only && !out) continue;
                if (stage_z) { decode_rows(h, m, z, nd, out, s); continue; }
                run_inference(h, m, false, nd, s);
                if (out) copy_out32(h, m, out, nd, s);
            }
            return;
        }
        ServeSlot sl;
        std::memset(&sl, 0, sizeof(sl));
        for (int c0 = 0; c0 < nd; c0 += h->B) {
            sl.z = z + (size_t)c0 * h->nz; sl.rows = std::min(h->B, nd - c0);
            for (int m = 0; m < h->M; ++m)
                sl.out[m] = (dst && dst[m]) ? dst[m] + (size_t)c0 * h->mods[m].n_in : h->at<float>(h->mods[m].out32);
            serve_call(h, serve_plan(h, serve_bucket(h, sl.rows)), sl, s);
        }
    }
};

// K samples of every input row, decoded in passes of at most `cap` rows: n_rows input rows x kb samples per pass (K >= cap: one
// row and cap samples, the row spanning several passes; else cap / K rows with all their samples).
struct SampleBlocks {
    int K, n_rows, kb;
    SampleBlocks(int K_, int cap) : K(K_), n_rows(K_ >= cap ? 1 : cap / std::max(K_, 1)), kb(K_ >= cap ? cap : K_) {}
    // body(k0, kc, nd): samples [k0, k0 + kc) of nj input rows = nd decoded rows
    template <typename F> void each(int nj, F&& body) const {
        for (int k0 = 0; k0 < K; k0 += kb) {
            const int kc = std::min(kb, K - k0);
            body(k0, kc, nj * kc);
        }
    }
};

// ---- gradient latent refinement (avae_complete; include/avae.h, avae_complete.h).  One pass over a chunk of <= batch_size rows:
//   cmpl_dec<k>      the decoders' hidden layers from the current z (grouped over the modalities, as fwd_dec<k>)
//   cmpl_out         output layers, p / x_hat as fp32 into out32 (the inference kind: no loss epilogue)
//   k_complete_out   element-masked output gradient into dO + recon_obs per (row, modality)
//   cmpl_bwd_out, cmpl_bwd_dec<k>   the training plan's decoder dgrad items (bwd_out, bwd_dec<k>), built again here from the same
//                    builders: the training launches also carry the latent item's [dmu | dlv] conversion and the cost item
//                    (step counter, lr_t), which must not run
//   cmpl_bwd_dz      dz_m = dD1 . V1^T as plain fp32 (the conv branch's K_DGRAD_F32 kind) into the scratch
//   k_complete_update   sum over modalities + prior, objective, Adam on z, new decoder inputs
// = 2 L + 4 launches for L hidden layers (8 for the reference's two).  The plan's rows are batch_size, whatever the chunk holds:
// the GEMM items are the training step's shapes, and rows beyond the chunk's are zeros that nobody reads.  No weight gradient,
// no write to the gradient buffer, theta or the optimiser state.
constexpr int kCompleteSizes[3] = {16, 4, 1};   // passes per captured graph

void complete_pass(avae_handle* h, avae_handle::Complete& cp, hipStream_t s) {
    run_launches(h, cp.fwd, s);
    timed_launch(h, s, "complete_out", [&] { launch_complete_out(h->cfg.compute_dtype, cp.args, s); });
    run_launches(h, cp.bwd, s);
    timed_launch(h, s, "complete_update", [&] { launch_complete_update(h->cfg.compute_dtype, cp.args, s); });
}

avae_handle::Complete& complete_plan(avae_handle* h) {
    avae_handle::Complete& cp = h->cmpl;
    if (cp.built) return cp;
    const int B = h->B, M = h->M, nz = h->nz, lddz = (int)rup(nz, 4);
    Bump b;
    const size_t off_call = b.take(sizeof(CompleteCall));
    const size_t off_z = b.take((size_t)B * nz * 4), off_m = b.take((size_t)B * nz * 4), off_v = b.take((size_t)B * nz * 4);
    const size_t off_recon = b.take((size_t)B * M * 4);
    size_t off_dz[kMaxMod] = {0, 0, 0, 0};
    for (int m = 0; m < M; ++m) off_dz[m] = b.take(rup(B, kRowAlign) * (size_t)lddz * 4);
    unsigned char* buf = static_cast<unsigned char*>(cp.buf.ensure(b.off, true));
    CompleteArgs& a = cp.args;
    std::memset(&a, 0, sizeof(a));
    a.call = reinterpret_cast<CompleteCall*>(buf + off_call);
    a.z32 = reinterpret_cast<float*>(buf + off_z); a.m = reinterpret_cast<float*>(buf + off_m); a.v = reinterpret_cast<float*>(buf + off_v);
    a.recon = reinterpret_cast<float*>(buf + off_recon);
    a.beta1 = h->cfg.beta1; a.beta2 = h->cfg.beta2; a.eps = h->cfg.adam_eps;
    a.n_mod = M; a.nz = nz; a.bucket = B;
    for (int m = 0; m < M; ++m) {
        const Mod& md = h->mods[m];
        a.Z[m] = h->at<void>(md.Z.rm); a.ldz[m] = md.Z.ld;
        a.out32[m] = h->at<float>(md.out32); a.ld32[m] = md.ld32;
        a.dO[m] = h->at<void>(md.dO.rm); a.lddo[m] = md.dO.ld;
        a.dz[m] = reinterpret_cast<float*>(buf + off_dz[m]); a.lddz[m] = lddz;
        a.n_in[m] = md.n_in; a.binary[m] = h->cfg.mod[m].binary ? 1 : 0; a.w[m] = h->cfg.mod[m].weight;
    }
    cp.items.clear(); cp.fwd.clear(); cp.bwd.clear();
    Builder bd(h, cp.items, B, false);
    Groups group{h, cp.items};
    int Lmax = 0;
    for (const Mod& md : h->mods) Lmax = std::max(Lmax, md.L);
    for (int k = 0; k < Lmax; ++k)
        group("cmpl_dec" + std::to_string(k + 1), cp.fwd, [&] {
            for (Mod& md : h->mods) if (k < md.L) cp.items.push_back(bd.fwd_hidden(k == 0 ? md.Z : md.D[k - 1], md.dec[k], md.D[k])); });
    group("cmpl_out", cp.fwd, [&] { for (int m = 0; m < M; ++m) cp.items.push_back(bd.fwd_out(h->mods[m], m, false)); });
    group("cmpl_bwd_out", cp.bwd, [&] {
        for (Mod& md : h->mods) cp.items.push_back(bd.dgrad_hidden(md.dO, md.outl, md.D.back(), md.dD.back())); });
    for (int k = Lmax - 1; k >= 1; --k)
        group("cmpl_bwd_dec" + std::to_string(k + 1), cp.bwd, [&] {
            for (Mod& md : h->mods) if (k < md.L) cp.items.push_back(bd.dgrad_hidden(md.dD[k], md.dec[k], md.D[k - 1], md.dD[k - 1])); });
    group("cmpl_bwd_dz", cp.bwd, [&] {
        for (int m = 0; m < M; ++m) {
            const Mod& md = h->mods[m];
            const Dense& d = md.dec[0];
            WorkItem w = gemm_item(K_DGRAD_F32, B, nz, bd.K_of(d.out), h->at<void>(md.dD[0].rm), md.dD[0].ld, h->at<void>(d.W), d.ldw);
            w.out0 = const_cast<float*>(a.dz[m]); w.ld0 = lddz;
            cp.items.push_back(w);
        } });
    if (h->cfg.use_graph) {
        try {
            for (int i = 0; i < 3; ++i)
                cp.g[i] = capture(h, [&](hipStream_t cs) { for (int j = 0; j < kCompleteSizes[i]; ++j) complete_pass(h, cp, cs); });
        } catch (...) { for (StepGraph& g : cp.g) g.release(); throw; }
    }
    cp.built = true;
    return cp;
}

// ---- masked steps: per-row modality presence (include/avae.h).  The masked twin of the step is built on first use: the forward
// launches with WorkItem::present pointing at the staged presence bytes in every loss and latent item, and their graphs.
void build_masked(avae_handle* h) {
    if (!h->masked.fwd.empty()) return;
    h->pres_set = (size_t)h->B * h->M;             // = the staging kernel's set stride (PrepArgs::pres_dst: set j at j * rows * M)
    unsigned char* pres = static_cast<unsigned char*>(h->pres_buf.ensure(h->pres_set * kMultiSteps, true));
    std::vector<Launch> mf = h->plain.fwd;
    int n_loss = 0, n_latent = 0;
    for (Launch& L : mf) {
        if (L.type != kGrouped || L.tn) continue;
        bool gated = false;
        for (int i = 0; i < L.args.n_items; ++i) {
            WorkItem& w = L.args.items[i];
            if (w.kind == K_FWD_OUT_LOSS) {
                int m = 0;
                while (m < h->M && w.aux0 != h->at<void>(h->mods[m].X32)) ++m;      // the item's modality: whose exact inputs it reads
                if (m == h->M) throw Err("internal error: a loss item of no modality");
                w.present = pres + m; w.present_ld = h->M;
                gated = true; ++n_loss;
            } else if (w.kind == K_LATENT) {
                w.present = pres; w.present_ld = h->M;
                gated = true; ++n_latent;
            }
        }
        // the kernels that carry the presence gate (TileGeom::masked): k_grouped's 4-wave tiles, its 8-wave loss tile and the small
        // nets' loss kernel.  Any other route of a loss or latent item would ignore the mask: refuse.
        if (gated && !tile_geom(L.cfg).masked)
            throw Err("masked training is not available on this plan: launch " + L.name + " (tile configuration " + std::to_string((int)L.cfg) +
                      ") carries a loss or latent item on a kernel without the presence gate");
    }
    if (n_loss != h->M || n_latent != 1) throw Err("internal error: the masked twin found " + std::to_string(n_loss) + " loss and " +
                                                   std::to_string(n_latent) + " latent items");
    for (Launch& L : mf) if (two_line_records(L)) L.desc_n = 0;      // the records know no presence bytes: the twin's launches stay by-value
    h->masked.fwd.swap(mf);
    if (h->cfg.use_graph) {
        try { capture_plan(h, h->masked, pres); } catch (...) { h->masked.fwd.clear(); throw; }      // the next masked call builds it again
    }
}

void check_masked_call(avae_handle* h, const char* what, const float* const* x_dev, const uint8_t* present_dev) {
    if (h->cfg.world_size > 1 || h->cfg.use_comm != AVAE_COMM_NONE || h->comm_on)
        throw Err(std::string(what) + ": masked steps run on one replica only (world_size 1, use_comm AVAE_COMM_NONE)");
    if (!x_dev) throw Err(std::string(what) + ": null x_dev");
    if (!present_dev) throw Err(std::string(what) + ": present_dev is null (unmasked calls go through the unmasked entry points)");
}

// The explicit encoder inputs of an _in call: a modality's input needs its target, and rows at least n_input wide.
void check_inputs(avae_handle* h, const char* what, const float* const* x_dev, const float* const* in_dev, const int32_t* in_ld) {
    if (!x_dev) throw Err(std::string(what) + ": null x_dev");
    for (int m = 0; in_dev && m < h->M; ++m) {
        if (!in_dev[m]) continue;
        if (!x_dev[m]) throw Err(std::string(what) + ": in_dev[" + std::to_string(m) + "] is set while x_dev[" + std::to_string(m) + "] is null");
        if (in_ld && in_ld[m] > 0 && in_ld[m] < h->mods[m].n_in)
            throw Err(std::string(what) + ": in_ld[" + std::to_string(m) + "] = " + std::to_string(in_ld[m]) + " is below n_input = " +
                      std::to_string(h->mods[m].n_in));
    }
}

// One single-replica step of plan p (present: the masked plan's presence bytes).  With a library-owned collective (plain plan only:
// masked calls refuse it) the step is staged and runs the bucketed pipeline instead.
void train_one(avae_handle* h, StepPlan& p, const float* const* x_dev, const int32_t* x_ld, const uint8_t* present, const float* eps_dev,
               const PrepIn& pin, hipStream_t s) {
    if (h->comm_on) {
        run_prep_batch(h, x_dev, x_ld, eps_dev, h->B, kTrainSalt, s, nullptr, 1, pin);
        dp_step(h, 0, s);
        return;
    }
    if (p.full.exec && !h->timing) {    // the whole step, staging kernel included, is one graph replay
        patch_prep(h, p.full, x_dev, x_ld, eps_dev, 1, present, pin);
        HIP_OK(hipGraphLaunch(p.full.exec, s));
        return;
    }
    run_prep_batch(h, x_dev, x_ld, eps_dev, h->B, kTrainSalt, s, present, 1, pin);
    step_body(h, p.fwd, s, 0);
    if (h->timing) {      // floor of the measurement: a one-store kernel (partial slot 0 is rewritten every step anyway)
        timed_launch(h, s, "_null_kernel", [&] { launch_fill(h->at<void>(h->off_partial), 4, 0u, 0, 1, 1, s); });
    }
}

// Batch i of a run of consecutive batches: rows [i*B, (i+1)*B) of every modality (a null one stays null), of its explicit encoder
// input, of the presence bytes and of eps.
struct BatchRun {
    const avae_handle* h;
    const float* const* x_dev;
    const int32_t* x_ld;
    const uint8_t* present;
    const float* eps_dev;
    const float* const* in_dev;
    const int32_t* in_ld;
    const float* x[kMaxMod] = {};
    const float* in[kMaxMod] = {};
    const uint8_t* pres = nullptr;
    const float* eps = nullptr;
    PrepIn pin() const { return PrepIn{in, in_ld, true}; }      // (a training run: the handle's corruption applies)
    void at(int i) {
        for (int m = 0; m < h->M; ++m) {
            const size_t ld = (x_ld && x_ld[m] > 0) ? (size_t)x_ld[m] : (size_t)h->mods[m].n_in;
            x[m] = x_dev[m] ? x_dev[m] + (size_t)i * h->B * ld : nullptr;
            const size_t ldi = (in_ld && in_ld[m] > 0) ? (size_t)in_ld[m] : (size_t)h->mods[m].n_in;
            in[m] = (in_dev && in_dev[m]) ? in_dev[m] + (size_t)i * h->B * ldi : nullptr;
        }
        pres = present ? present + (size_t)i * h->B * h->M : nullptr;
        eps = eps_dev ? eps_dev + (size_t)i * h->B * h->nz : nullptr;
    }
};

// Replays runs of kMultiSizes[gi] batches (16, then 4) through g[gi] while ready(gi); returns the first batch not replayed.
template <typename Ready>
int replay_runs(avae_handle* h, StepGraph (&g)[2], BatchRun& b, int n_steps, hipStream_t s, Ready&& ready) {
    int i = 0;
    for (int gi = 0; gi < 2; ++gi)
        for (; i + kMultiSizes[gi] <= n_steps && ready(gi); i += kMultiSizes[gi]) {
            b.at(i);
            patch_prep(h, g[gi], b.x, b.x_ld, b.eps, kMultiSizes[gi], b.pres, b.pin());
            HIP_OK(hipGraphLaunch(g[gi].exec, s));
        }
    return i;
}

// n_steps consecutive batches through plan p (avae_train_steps, avae_train_steps_masked)
void train_steps(avae_handle* h, StepPlan& p, int n_steps, const float* const* x_dev, const int32_t* x_ld, const float* const* in_dev,
                 const int32_t* in_ld, const uint8_t* present, const float* eps_dev, float* cost_host, hipStream_t s) {
    BatchRun b{h, x_dev, x_ld, present, eps_dev, in_dev, in_ld};
    int i = 0;
    if (h->comm_on) {               // data parallel: batches staged kMultiSteps at a time, then backward -> all-reduce -> Adam per bucket and step
        // Runs of 16 (then 4) steps as ONE captured graph -- staging kernel, segments, ncclAllReduce on the comm stream (it
        // joins the capture through the events), Adam per bucket -- so that the host is out of the loop exactly as in the
        // single-replica path.  Captured on first use; if RCCL refuses capture on this stack the host steps the same pipeline.
        if (h->cfg.use_graph && !h->timing)
            i = replay_runs(h, h->g_dpm, b, n_steps, s, [&](int gi) {
                if (h->dp_graph_failed) return false;
                if (h->g_dpm[gi].exec) return true;
                std::vector<const float*> x0(h->M, h->at<float>(h->mods[0].X32));
                try {
                    h->g_dpm[gi] = capture(h, [&](hipStream_t cs) {
                        run_prep_batch(h, x0.data(), nullptr, nullptr, h->B, kTrainSalt, cs, nullptr, kMultiSizes[gi]);
                        for (int j = 0; j < kMultiSizes[gi]; ++j) dp_step(h, j, cs, true);
                    }, true);
                } catch (const std::exception& e) {
                    h->dp_graph_failed = true;
                    (void)hipGetLastError();
                    if (h->sw.debug_dp) std::fprintf(stderr, "[avae] data-parallel graph capture failed (%s): host-stepped pipeline\n", e.what());
                    return false;
                }
                return true;
            });
        for (; i < n_steps; i += kMultiSteps) {
            const int n = std::min(kMultiSteps, n_steps - i);
            b.at(i);
            run_prep_batch(h, b.x, x_ld, b.eps, h->B, kTrainSalt, s, nullptr, n, b.pin());
            for (int j = 0; j < n; ++j) dp_step(h, j, s);
        }
    } else {
        if (!h->timing) i = replay_runs(h, p.multi, b, n_steps, s, [&](int gi) { return p.multi[gi].exec != nullptr; });
        for (; i < n_steps; ++i) {
            b.at(i);
            train_one(h, p, b.x, x_ld, b.pres, b.eps, b.pin(), s);
        }
    }
    if (h->clip_on) h->clip_steps += n_steps;
    if (h->sched_on) h->sched_steps += n_steps;
    fetch_cost(h, cost_host, true, s);
}

// Forward + cost of one batch through plan p, no update (avae_eval_cost, avae_eval_cost_masked).
// in_dev / in_ld: explicit encoder inputs (avae_eval_cost_in); the handle's corruption never applies to an evaluation.
void eval_cost(avae_handle* h, StepPlan& p, const float* const* x_dev, const int32_t* x_ld, const float* const* in_dev, const int32_t* in_ld,
               const uint8_t* present, const float* eps_dev, float* cost_host, hipStream_t s) {
    run_prep_batch(h, x_dev, x_ld, eps_dev, h->B, 0x6576616cull /*eval*/ | (unsigned long long)next_draw(h, eps_dev) << 34, s, present, 1,
                   PrepIn{in_dev, in_ld, false});
    if (p.eval.exec && !h->timing) HIP_OK(hipGraphLaunch(p.eval.exec, s));
    else { run_launches(h, p.fwd, s); run_launch(h, h->cost_only, s, nullptr, -1); }
    fetch_cost(h, cost_host, false, s);
}

// Every call that trains or stages a training step: refused while the shadows hold the average.
void require_live(const avae_handle* h, const char* who) {
    if (h->averaged)
        throw Err(std::string(who) + ": the handle runs on the averaged weights; call avae_use_averaged(h, 0) before training");
}

void ema_to_host(avae_handle* h, std::vector<float>& host) {
    host.resize(h->P_int);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(host.data(), h->ema_avg(), h->P_int * 4, hipMemcpyDeviceToHost));
}
void host_to_ema(avae_handle* h, const std::vector<float>& host) {
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(h->ema_avg(), host.data(), h->P_int * 4, hipMemcpyHostToDevice));
}
// average <- theta, on the device (padding included: zero in both)
void ema_from_theta(avae_handle* h) {
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(h->ema_avg(), h->at<void>(h->off_theta), h->P_int * 4, hipMemcpyDeviceToDevice));
    HIP_OK(hipDeviceSynchronize());
}

// The mode-1 launch from the average (on) or from theta (off): the shadows every forward launch reads.
void use_averaged(avae_handle* h, bool on) {
    if (on && !h->ema_on) throw Err("avae_use_averaged: parameter averaging is off (avae_set_ema)");
    if (on == h->averaged) return;
    HIP_OK(hipDeviceSynchronize());
    run_adam(h, 1, nullptr, -1, on);
    HIP_OK(hipDeviceSynchronize());
    h->averaged = on;
}

void set_ema(avae_handle* h, float decay, int32_t warmup) {
    if (!(decay >= 0.0f && decay < 1.0f)) throw Err("avae_set_ema: decay must be in (0, 1), or 0 to switch averaging off");
    if (warmup != 0 && warmup != 1) throw Err("avae_set_ema: warmup must be 0 or 1");
    const bool on = decay > 0.0f;
    HIP_OK(hipDeviceSynchronize());             // a rare call: enqueued work keeps the setting it was enqueued with
    if (!on && !h->ema_buf.p) return;           // never switched on
    if (!on && h->averaged) use_averaged(h, false);
    h->ema_buf.ensure(sizeof(EmaState) + h->P_int * sizeof(float));
    if (on) {
        EmaState v;
        std::memset(&v, 0, sizeof(v));
        v.decay = decay; v.warmup = warmup;
        HIP_OK(hipMemcpy(h->ema_buf.p, &v, sizeof(v), hipMemcpyHostToDevice));
        h->ema_decay = decay; h->ema_warmup = warmup;
    }
    // new values only: k_adam reads them from the device (unless an earlier capture failed and left the plan without graphs)
    if (on == h->ema_on && (!h->cfg.use_graph || h->plain.full.exec)) return;
    if (on && !h->ema_on) ema_from_theta(h);    // the average starts at the current parameters
    // on <-> off: the step's tail changes, so every graph that holds an optimiser goes; the data-parallel segment graphs hold
    // none and stay, g_dpm is captured again by its next use
    h->plain.full.release(); h->plain.multi[0].release(); h->plain.multi[1].release();
    h->masked.full.release(); h->masked.multi[0].release(); h->masked.multi[1].release();
    for (StepGraph& g : h->g_dpm) g.release();
    h->ema_on = on;
    if (h->cfg.use_graph) {
        capture_steps(h, h->plain, nullptr);
        if (!h->masked.fwd.empty()) capture_steps(h, h->masked, h->pres_buf.as<unsigned char>());
    }
}

// Frees whatever the handle holds (a partly created one included), then the handle.
void destroy_handle(avae_handle* h) {
    int prev_dev = -1;
    if (hipGetDevice(&prev_dev) != hipSuccess) prev_dev = -1;
    (void)hipSetDevice(h->cfg.device);
    (void)hipDeviceSynchronize();
    h->plain.release();
    h->masked.release();
    for (StepGraph& g : h->g_dpm) g.release();
    for (std::vector<StepGraph>& v : h->g_dp) for (StepGraph& g : v) g.release();
    for (avae_handle::Serve& sv : h->serve) if (sv.graph) (void)hipGraphExecDestroy(sv.graph);
    for (StepGraph& g : h->cmpl.g) g.release();
    if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
    if (h->comm) { try { (void)Rccl::get().destroy(h->comm); } catch (...) {} }
    for (int r = 0; r < kMaxWorld; ++r) if (h->ipc_opened[r] && h->ipc_peer[r]) (void)hipIpcCloseMemHandle(h->ipc_peer[r]);
    if (h->ipc_block) (void)hipFree(h->ipc_block);
    for (int b = 0; b < 2; ++b) { if (h->ev_grad[b]) (void)hipEventDestroy(h->ev_grad[b]); if (h->ev_red[b]) (void)hipEventDestroy(h->ev_red[b]); }
    if (h->comm_stream) (void)hipStreamDestroy(h->comm_stream);
    for (TimingRec& r : h->trecs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    if (h->own_ws && h->ws) (void)hipFree(h->ws);
    const int dev = h->cfg.device;
    delete h;                                   // (with its DevBuf scratch, while the handle's device is still current)
    if (prev_dev >= 0 && prev_dev != dev) (void)hipSetDevice(prev_dev);
}

// ---- the latent-space features (DESIGN.md sections 18-23): what their entry points (in the C ABI below) share
// A *_plan query: it has no handle, so what it throws goes where avae_create's errors go.
template <typename F> int plan_query(const avae_config* cfg, F&& query) {
    try {
        if (!cfg) throw Err("null argument");
        check_config(*cfg);
        query();
        return 0;
    } catch (const std::exception& e) { g_create_error = e.what(); return 2; }
}
template <typename T> void put(T* out, T v) { if (out) *out = v; }     // an optional output
void need(const std::string& w, const void* p, const char* name, const char* why = nullptr) {
    if (!p) throw Err(w + ": " + name + " is NULL" + (why ? " (" + std::string(why) + ")" : std::string()));
}
void check_rows(const std::string& w, long long rows, const char* name) {
    if (rows < 0) throw Err(w + ": " + name + " must be >= 0");
}
bool check_metric(const std::string& w, int32_t metric) {             // true: AVAE_METRIC_SYMKL
    if (metric != AVAE_METRIC_SYMKL && metric != AVAE_METRIC_L2)
        throw Err(w + ": metric = " + std::to_string(metric) + " is neither AVAE_METRIC_SYMKL nor AVAE_METRIC_L2");
    return metric == AVAE_METRIC_SYMKL;
}
const char* const kNeedsLogvar = "AVAE_METRIC_SYMKL reads the log-variances";
// The handle's scratch of a feature, allocated once at its bound.  A plan beyond the bound (lds_bytes given: or beyond a CU's LDS)
// is a mistake of the plan, not of the caller.
template <typename T>
T* scratch_of(DevBuf& buf, const std::string& w, size_t need_bytes, size_t bound_bytes, size_t lds_bytes = 0) {
    if (need_bytes > bound_bytes || lds_bytes > kMaxDynLds)
        throw Err("internal error: " + w + " plans more " + (lds_bytes ? "scratch or LDS" : "scratch") + " than its bound");
    return static_cast<T*>(buf.ensure(bound_bytes));
}
template <typename T> T zeroed() { T a; std::memset(&a, 0, sizeof(a)); return a; }   // kernel arguments start as zeros, pads included

}  // namespace

// ============================================================================= C ABI
extern "C" {

int avae_workspace_bytes(const avae_config* cfg, size_t* bytes) {
    try {
        if (!cfg || !bytes) throw Err("null argument");
        check_config(*cfg);
        avae_handle tmp;
        tmp.cfg = *cfg;
        tmp.sw = read_switches();
        plan_memory(&tmp);
        *bytes = tmp.ws_bytes;
        return 0;
    } catch (const std::exception& e) { g_create_error = e.what(); return 2; }
}

int avae_create(const avae_config* cfg, avae_handle** out) {
    avae_handle* h = nullptr;
    try {
        if (!cfg || !out) throw Err("null argument");
        check_config(*cfg);
        h = new avae_handle();
        h->cfg = *cfg;
        h->sw = read_switches();
        if (h->sw.debug_sync) h->cfg.use_graph = 0;
        if (h->cfg.beta1 == 0.f && h->cfg.beta2 == 0.f && h->cfg.adam_eps == 0.f) { h->cfg.beta1 = 0.9f; h->cfg.beta2 = 0.999f; h->cfg.adam_eps = 1e-8f; }
        int ndev = 0;
        HIP_OK(hipGetDeviceCount(&ndev));
        if (ndev < 1) throw Err("no HIP device: libavae has no CPU fallback");
        if (h->cfg.device < 0 || h->cfg.device >= ndev) throw Err("device ordinal out of range");
        DeviceGuard dg(h->cfg.device);
        hipDeviceProp_t prop;
        HIP_OK(hipGetDeviceProperties(&prop, h->cfg.device));
        if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
            throw Err(std::string("libavae is built for gfx950 only; device is ") + prop.gcnArchName);
        plan_memory(h);
        if (cfg->workspace) {
            if (cfg->workspace_bytes < h->ws_bytes) throw Err("workspace too small");
            if (reinterpret_cast<uintptr_t>(cfg->workspace) % 256) throw Err("workspace must be 256-byte aligned");
            h->ws = reinterpret_cast<unsigned char*>(cfg->workspace);
        } else {
            HIP_OK(hipMalloc(reinterpret_cast<void**>(&h->ws), h->ws_bytes));
            h->own_ws = true;
        }
        HIP_OK(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
        init_device(h);
        if (h->cfg.use_comm) comm_init(h);
        *out = h;
        return 0;
    } catch (const std::exception& e) {
        g_create_error = e.what();
        if (h) destroy_handle(h);
        return 2;
    }
}

void avae_destroy(avae_handle* h) {
    if (h) destroy_handle(h);
}

const char* avae_last_error(const avae_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int avae_param_count(const avae_handle* h, size_t* n) {
    if (!h || !n) return 1;
    *n = h->P_flat;
    return 0;
}

int avae_get_params(avae_handle* h, float* host_dst) {
    return guarded(h, [&] { std::vector<float> I; master_to_host(h, h->off_theta, I); convert_params<false>(h, host_dst, I.data()); });
}

int avae_set_params(avae_handle* h, const float* host_src) {
    return guarded(h, [&] {
        std::vector<float> I(h->P_int, 0.0f);
        convert_params<true>(h, const_cast<float*>(host_src), I.data());
        host_to_master(h, h->off_theta, I);
        run_adam(h, 1, nullptr);          // rebuild the compute-dtype shadows W / W^T (from theta: avae_use_averaged is off after this)
        HIP_OK(hipDeviceSynchronize());
        h->averaged = false;
    });
}

int avae_get_grads(avae_handle* h, float* host_dst) {
    return guarded(h, [&] { std::vector<float> I; master_to_host(h, h->off_g, I); convert_params<false>(h, host_dst, I.data()); });
}

int avae_get_opt_state(avae_handle* h, float* host_m, float* host_v, int64_t* step) {
    return guarded(h, [&] {
        std::vector<float> I;
        if (host_m) { master_to_host(h, h->off_m, I); convert_params<false>(h, host_m, I.data()); }
        if (host_v) { master_to_host(h, h->off_v, I); convert_params<false>(h, host_v, I.data()); }
        if (step) { long long st = 0; HIP_OK(hipDeviceSynchronize()); HIP_OK(hipMemcpy(&st, &h->state()->step, sizeof(st), hipMemcpyDeviceToHost)); *step = st; }
    });
}

int avae_set_opt_state(avae_handle* h, const float* host_m, const float* host_v, int64_t step) {
    return guarded(h, [&] {
        std::vector<float> I(h->P_int, 0.0f);
        if (host_m) { convert_params<true>(h, const_cast<float*>(host_m), I.data()); host_to_master(h, h->off_m, I); }
        if (host_v) { std::fill(I.begin(), I.end(), 0.0f); convert_params<true>(h, const_cast<float*>(host_v), I.data()); host_to_master(h, h->off_v, I); }
        long long st = step;
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(&h->state()->step, &st, sizeof(st), hipMemcpyHostToDevice));
    });
}

// Data-parallel runs of consecutive batches: one staging launch for up to kMultiSteps batches, then per step
// backward on its staging set -> (caller's all-reduce) -> apply.
int avae_stage_batches_in(avae_handle* h, int32_t n_steps, const float* const* x_dev, const int32_t* x_ld, const float* const* in_dev,
                          const int32_t* in_ld, const float* eps_dev, void* stream) {
    return guarded(h, [&] {
        require_live(h, "avae_stage_batches");
        if (n_steps < 1 || n_steps > kMultiSteps) throw Err("avae_stage_batches: n_steps must be in [1," + std::to_string(kMultiSteps) + "]");
        check_inputs(h, "avae_stage_batches_in", x_dev, in_dev, in_ld);
        run_prep_batch(h, x_dev, x_ld, eps_dev, h->B, kTrainSalt, on_stream(h, stream), nullptr, n_steps, PrepIn{in_dev, in_ld, true});
    });
}

int avae_stage_batches(avae_handle* h, int32_t n_steps, const float* const* x_dev, const int32_t* x_ld, const float* eps_dev, void* stream) {
    return avae_stage_batches_in(h, n_steps, x_dev, x_ld, nullptr, nullptr, eps_dev, stream);
}

int avae_train_step(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, const float* eps_dev, float* cost_host, void* stream) {
    return guarded(h, [&] {
        require_live(h, "avae_train_step");
        hipStream_t s = on_stream(h, stream);
        train_one(h, h->plain, x_dev, x_ld, nullptr, eps_dev, PrepIn{nullptr, nullptr, true}, s);
        if (h->clip_on) ++h->clip_steps;
        if (h->sched_on) ++h->sched_steps;
        fetch_cost(h, cost_host, true, s);
    });
}

int avae_train_steps_in(avae_handle* h, int32_t n_steps, const float* const* x_dev, const int32_t* x_ld, const float* const* in_dev,
                        const int32_t* in_ld, const uint8_t* present_dev, const float* eps_dev, float* cost_host, void* stream) {
    return guarded(h, [&] {
        require_live(h, "avae_train_steps_in");
        if (present_dev) check_masked_call(h, "avae_train_steps_in", x_dev, present_dev);
        if (n_steps < 1) throw Err("avae_train_steps_in: n_steps must be >= 1");
        check_inputs(h, "avae_train_steps_in", x_dev, in_dev, in_ld);
        if (present_dev) build_masked(h);
        train_steps(h, present_dev ? h->masked : h->plain, n_steps, x_dev, x_ld, in_dev, in_ld, present_dev, eps_dev, cost_host,
                    on_stream(h, stream));
    });
}

int avae_train_steps(avae_handle* h, int32_t n_steps, const float* const* x_dev, const int32_t* x_ld, const float* eps_dev,
                     float* cost_host, void* stream) {
    return guarded(h, [&] {
        require_live(h, "avae_train_steps");
        if (n_steps < 1) throw Err("avae_train_steps: n_steps must be >= 1");
        train_steps(h, h->plain, n_steps, x_dev, x_ld, nullptr, nullptr, nullptr, eps_dev, cost_host, on_stream(h, stream));
    });
}

int avae_set_corruption(avae_handle* h, const avae_corruption* c) {
    return guarded(h, [&] {
        avae_corruption v{};
        unsigned thr[kMaxMod] = {};
        if (c) v = *c;
        for (int m = 0; m < AVAE_MAX_MODALITIES; ++m) {
            const std::string at = "[" + std::to_string(m) + "]";
            if (!(v.drop_prob[m] >= 0.0f && v.drop_prob[m] < 1.0f)) throw Err("avae_set_corruption: drop_prob" + at + " must be in [0, 1)");
            if (!std::isfinite(v.drop_value[m])) throw Err("avae_set_corruption: drop_value" + at + " must be finite");
            if (!(v.noise_std[m] >= 0.0f) || !std::isfinite(v.noise_std[m]))
                throw Err("avae_set_corruption: noise_std" + at + " must be finite and >= 0");
            thr[m] = (unsigned)std::floor((double)v.drop_prob[m] * 16777216.0);
        }
        h->corr = v;
        std::memcpy(h->drop_thr, thr, sizeof(thr));
    });
}

int avae_set_grad_clip(avae_handle* h, float max_norm, int32_t skip_nonfinite) {
    return guarded(h, [&] {
        if (!(max_norm >= 0.0f)) throw Err("avae_set_grad_clip: max_norm must be >= 0 (0 = no clipping, +inf = monitor only)");
        if (skip_nonfinite != 0 && skip_nonfinite != 1) throw Err("avae_set_grad_clip: skip_nonfinite must be 0 or 1");
        const bool on = max_norm > 0.0f || skip_nonfinite != 0;
        HIP_OK(hipDeviceSynchronize());             // a rare call: enqueued work keeps the setting it was enqueued with
        if (!on && !h->clip_buf.p) return;          // never switched on
        ClipState* cs = static_cast<ClipState*>(h->clip_buf.ensure(sizeof(ClipState), true));
        struct { float max_norm; int skip; } v = {max_norm, skip_nonfinite};
        static_assert(offsetof(ClipState, skip_nonfinite) == sizeof(float), "the two settings are adjacent");
        HIP_OK(hipMemcpy(cs, &v, sizeof(v), hipMemcpyHostToDevice));
        // new values only: the kernels read them from the device (unless an earlier capture failed and left the plan without graphs)
        if (on == h->clip_on && (!h->cfg.use_graph || h->plain.full.exec)) return;
        // on <-> off: the step's tail changes, so every graph that holds an optimiser goes; the data-parallel segment graphs hold
        // none and stay, g_dpm is captured again by its next use
        h->plain.full.release(); h->plain.multi[0].release(); h->plain.multi[1].release();
        h->masked.full.release(); h->masked.multi[0].release(); h->masked.multi[1].release();
        for (StepGraph& g : h->g_dpm) g.release();
        h->clip_on = on;
        if (on) h->clip_steps = 0;
        if (h->cfg.use_graph) {
            capture_steps(h, h->plain, nullptr);
            if (!h->masked.fwd.empty()) capture_steps(h, h->masked, h->pres_buf.as<unsigned char>());
        }
    });
}

int avae_grad_norm_history(avae_handle* h, int32_t n, float* host_norms, int64_t* last_step, int64_t* n_skipped) {
    return guarded(h, [&] {
        if (n < 0 || n > kCostHist) throw Err("avae_grad_norm_history: n must be in [0, " + std::to_string(kCostHist) + "]");
        if (n > 0 && !host_norms) throw Err("avae_grad_norm_history: null host_norms");
        if ((long long)n > (h->clip_on ? h->clip_steps : 0))
            throw Err("avae_grad_norm_history: " + std::to_string(n) + " norms asked for, " + std::to_string(h->clip_on ? h->clip_steps : 0) +
                      " steps submitted since clipping was switched on");
        HIP_OK(hipDeviceSynchronize());
        comm_check_error(h);
        long long step = 0;
        HIP_OK(hipMemcpy(&step, &h->state()->step, sizeof(step), hipMemcpyDeviceToHost));
        long long skipped = 0;
        if (h->clip_buf.p) {
            std::vector<unsigned char> buf(sizeof(ClipState));
            HIP_OK(hipMemcpy(buf.data(), h->clip_buf.p, sizeof(ClipState), hipMemcpyDeviceToHost));
            const ClipState* cs = reinterpret_cast<const ClipState*>(buf.data());
            if (step < n) throw Err("avae_grad_norm_history: fewer steps applied than requested");
            for (int i = 0; i < n; ++i) host_norms[i] = cs->norm_hist[(step - n + i) % kCostHist];
            skipped = cs->n_skipped;
        }
        if (last_step) *last_step = step;
        if (n_skipped) *n_skipped = skipped;
    });
}

int avae_set_ema(avae_handle* h, float decay, int32_t warmup) {
    return guarded(h, [&] { set_ema(h, decay, warmup); });
}

int avae_get_ema(avae_handle* h, float* host_dst) {
    return guarded(h, [&] {
        if (!h->ema_on) throw Err("avae_get_ema: parameter averaging is off (avae_set_ema)");
        if (!host_dst) throw Err("avae_get_ema: null host_dst");
        std::vector<float> I;
        ema_to_host(h, I);
        convert_params<false>(h, host_dst, I.data());
    });
}

int avae_set_ema_params(avae_handle* h, const float* host_src) {
    return guarded(h, [&] {
        if (!h->ema_on) throw Err("avae_set_ema_params: parameter averaging is off (avae_set_ema)");
        if (!host_src) throw Err("avae_set_ema_params: null host_src");
        std::vector<float> I(h->P_int, 0.0f);
        convert_params<true>(h, const_cast<float*>(host_src), I.data());
        host_to_ema(h, I);
        if (h->averaged) { run_adam(h, 1, nullptr, -1, true); HIP_OK(hipDeviceSynchronize()); }      // the shadows follow
    });
}

int avae_use_averaged(avae_handle* h, int32_t on) {
    return guarded(h, [&] {
        if (on != 0 && on != 1) throw Err("avae_use_averaged: on must be 0 or 1");
        use_averaged(h, on != 0);
    });
}

int avae_set_schedule(avae_handle* h, const avae_schedule* kl, const avae_schedule* assoc, const avae_schedule* lr) {
    return guarded(h, [&] {
        const avae_schedule* in[3] = {kl, assoc, lr};
        static const char* const names[3] = {"kl", "assoc", "lr"};
        avae_schedule sc[3];
        bool on = false;
        for (int q = 0; q < 3; ++q) {
            std::memset(&sc[q], 0, sizeof(sc[q]));
            if (!in[q] || in[q]->kind == AVAE_SCHED_NONE) continue;
            check_schedule(*in[q], std::string("avae_set_schedule: ") + names[q]);
            sc[q] = canonical_schedule(*in[q]);
            on = true;
        }
        HIP_OK(hipDeviceSynchronize());             // a rare call: enqueued work keeps the schedules it was enqueued with
        if (!on && !h->sched_buf.p) return;         // never switched on
        SchedState* ss = static_cast<SchedState*>(h->sched_buf.ensure(sizeof(SchedState), true));
        static_assert(offsetof(SchedState, sched) == 0 && offsetof(SchedState, lambda0) == sizeof(sc) &&
                      offsetof(SchedState, lr0) == sizeof(sc) + sizeof(float), "the settings lead the device state");
        struct { avae_schedule sc[3]; float lambda0, lr0; } v;
        std::memcpy(v.sc, sc, sizeof(sc));
        v.lambda0 = h->cfg.assoc_lambda; v.lr0 = h->cfg.learning_rate;
        HIP_OK(hipMemcpy(ss, &v, sizeof(sc) + 2 * sizeof(float), hipMemcpyHostToDevice));
        // new schedules only: the staging launch reads them from the device (unless an earlier capture failed and left the plan without graphs)
        if (on == h->sched_on && (!h->cfg.use_graph || h->plain.full.exec)) return;
        // on <-> off: the staging instance and the latent / cost items' arguments change, so every graph that holds a training launch
        // goes (the evaluation graphs hold neither and stay); the data-parallel graphs are captured again by their next use
        h->plain.full.release(); h->plain.multi[0].release(); h->plain.multi[1].release();
        h->masked.full.release(); h->masked.multi[0].release(); h->masked.multi[1].release();
        for (StepGraph& g : h->g_dpm) g.release();
        for (std::vector<StepGraph>& gv : h->g_dp) for (StepGraph& g : gv) g.release();
        h->sched_on = on;
        if (on) h->sched_steps = 0;
        if (h->cfg.use_graph) {
            capture_steps(h, h->plain, nullptr);
            if (!h->masked.fwd.empty()) capture_steps(h, h->masked, h->pres_buf.as<unsigned char>());
        }
    });
}

int avae_schedule_value(const avae_schedule* schedule, int64_t step, float* out) {
    try {
        if (!out) throw Err("avae_schedule_value: null out");
        if (step < 1) throw Err("avae_schedule_value: step must be >= 1 (the number the first update gets)");
        if (!schedule || schedule->kind == AVAE_SCHED_NONE) { *out = 1.0f; return 0; }
        check_schedule(*schedule, "avae_schedule_value: schedule");
        *out = schedule_value(canonical_schedule(*schedule), (long long)step);
        return 0;
    } catch (const std::exception& e) { g_create_error = e.what(); return 2; }
}

int avae_hyper_history(avae_handle* h, int32_t n, float* host_dst, int64_t* last_step) {
    return guarded(h, [&] {
        if (n < 0 || n > kCostHist) throw Err("avae_hyper_history: n must be in [0, " + std::to_string(kCostHist) + "]");
        if (n > 0 && !host_dst) throw Err("avae_hyper_history: null host_dst");
        const long long have = h->sched_on ? h->sched_steps : 0;
        if ((long long)n > have)
            throw Err("avae_hyper_history: " + std::to_string(n) + " steps asked for, " + std::to_string(have) +
                      " steps submitted since a schedule was switched on");
        HIP_OK(hipDeviceSynchronize());
        comm_check_error(h);
        long long step = 0;
        HIP_OK(hipMemcpy(&step, &h->state()->step, sizeof(step), hipMemcpyDeviceToHost));
        if (n > 0) {
            if (step < n) throw Err("avae_hyper_history: fewer steps applied than requested");
            std::vector<float> ring((size_t)kCostHist * 3);
            HIP_OK(hipMemcpy(ring.data(), reinterpret_cast<const unsigned char*>(h->sched_buf.p) + offsetof(SchedState, hist),
                             ring.size() * sizeof(float), hipMemcpyDeviceToHost));
            for (int i = 0; i < n; ++i) std::memcpy(host_dst + 3 * (size_t)i, &ring[3 * (size_t)((step - n + i) % kCostHist)], 3 * sizeof(float));
        }
        if (last_step) *last_step = step;
    });
}

int avae_train_steps_masked(avae_handle* h, int32_t n_steps, const float* const* x_dev, const int32_t* x_ld, const uint8_t* present_dev,
                            const float* eps_dev, float* cost_host, void* stream) {
    return guarded(h, [&] {
        require_live(h, "avae_train_steps_masked");
        check_masked_call(h, "avae_train_steps_masked", x_dev, present_dev);
        if (n_steps < 1) throw Err("avae_train_steps_masked: n_steps must be >= 1");
        build_masked(h);
        train_steps(h, h->masked, n_steps, x_dev, x_ld, nullptr, nullptr, present_dev, eps_dev, cost_host, on_stream(h, stream));
    });
}

int avae_eval_cost_masked(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, const uint8_t* present_dev, const float* eps_dev,
                          float* cost_host, void* stream) {
    return guarded(h, [&] {
        check_masked_call(h, "avae_eval_cost_masked", x_dev, present_dev);
        build_masked(h);
        eval_cost(h, h->masked, x_dev, x_ld, nullptr, nullptr, present_dev, eps_dev, cost_host, on_stream(h, stream));
    });
}

int avae_eval_cost_in(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, const float* const* in_dev, const int32_t* in_ld,
                      const uint8_t* present_dev, const float* eps_dev, float* cost_host, void* stream) {
    return guarded(h, [&] {
        if (present_dev) check_masked_call(h, "avae_eval_cost_in", x_dev, present_dev);
        check_inputs(h, "avae_eval_cost_in", x_dev, in_dev, in_ld);
        if (present_dev) build_masked(h);
        eval_cost(h, present_dev ? h->masked : h->plain, x_dev, x_ld, in_dev, in_ld, present_dev, eps_dev, cost_host, on_stream(h, stream));
    });
}

int avae_grad_buffer(avae_handle* h, float** dev_ptr, size_t* n_floats) {
    if (!h || !dev_ptr || !n_floats) return 1;
    *dev_ptr = h->grad();
    *n_floats = h->P_int + 1;     // gradient (internal padded layout) + the cost slot
    return 0;
}

int avae_dp_plan(const avae_config* cfg, int32_t* n_buckets, int32_t* n_ranges, int64_t* offs, int64_t* counts) {
    try {
        if (!cfg || !n_buckets || !n_ranges || !offs || !counts) throw Err("null argument");
        check_config(*cfg);
        avae_handle tmp;
        tmp.cfg = *cfg;
        tmp.sw = read_switches();
        plan_memory(&tmp);
        std::vector<avae_handle::Range> r[2];
        int nb = 0;
        dp_ranges(&tmp, &nb, r);
        *n_buckets = nb;
        int k = 0;
        for (int b = 0; b < 2; ++b) {
            n_ranges[b] = (int32_t)r[b].size();
            for (const avae_handle::Range& x : r[b]) { offs[k] = (int64_t)x.off; counts[k] = (int64_t)x.count; ++k; }
        }
        return 0;
    } catch (const std::exception& e) { g_create_error = e.what(); return 2; }
}

int avae_dp_backward(avae_handle* h, int32_t j, int32_t bucket, void* stream) {
    return guarded(h, [&] { require_live(h, "avae_dp_backward"); dp_segment(h, j, bucket, on_stream(h, stream)); });
}

int avae_dp_apply(avae_handle* h, int32_t bucket, float* cost_host, void* stream) {
    return guarded(h, [&] {
        require_live(h, "avae_dp_apply");
        if (bucket < 0 || bucket >= h->n_buckets) throw Err("data-parallel bucket out of range");
        hipStream_t s = on_stream(h, stream);
        if (h->clip_on && bucket == 0) { run_grad_sumsq(h, s); ++h->clip_steps; }      // over the whole buffer: both all-reduces come before apply(0); apply(1) reuses the partials
        if (h->sched_on && bucket == 0) ++h->sched_steps;
        run_adam(h, 0, s, h->n_buckets == 1 ? -1 : bucket);
        fetch_cost(h, cost_host, true, s);
    });
}

int avae_comm_unique_id(void* id128) {
    try {
        if (!id128) throw Err("null argument");
        NCCL_OK(Rccl::get().get_id(id128));
        return 0;
    } catch (const std::exception& e) { g_create_error = e.what(); return 2; }
}

int avae_comm_ipc_handle(avae_handle* h, void* handle_out) {
    return guarded(h, [&] {
        if (!handle_out) throw Err("null argument");
        if (!h->ipc_block) throw Err("avae_comm_ipc_handle: the replica was not created with use_comm = AVAE_COMM_IPC");
        IpcHandleBytes hb;
        std::memset(&hb, 0, sizeof(hb));
        HIP_OK(hipIpcGetMemHandle(&hb.mem, h->ipc_block));
        hb.bytes = h->ipc_bytes; hb.raw_ptr = reinterpret_cast<uint64_t>(h->ipc_block); hb.layout = ipc_layout_word(h);
        hb.rank = h->cfg.rank; hb.world = h->cfg.world_size; hb.pid = (int32_t)getpid(); hb.magic = kIpcMagic;
        std::memset(handle_out, 0, AVAE_IPC_HANDLE_BYTES);
        std::memcpy(handle_out, &hb, sizeof(hb));
    });
}

int avae_comm_ipc_attach(avae_handle* h, const void* handles_by_rank) {
    return guarded(h, [&] {
        if (!handles_by_rank) throw Err("null argument");
        if (!h->ipc_block) throw Err("avae_comm_ipc_attach: the replica was not created with use_comm = AVAE_COMM_IPC");
        if (h->ipc_attached && h->cfg.world_size > 1) throw Err("avae_comm_ipc_attach: already attached");
        const unsigned char* raw = reinterpret_cast<const unsigned char*>(handles_by_rank);
        for (int r = 0; r < h->cfg.world_size; ++r) {
            IpcHandleBytes hb;
            std::memcpy(&hb, raw + (size_t)r * AVAE_IPC_HANDLE_BYTES, sizeof(hb));
            if (hb.magic != kIpcMagic || hb.rank != r || hb.world != h->cfg.world_size)
                throw Err("avae_comm_ipc_attach: entry " + std::to_string(r) + " is not rank " + std::to_string(r) + "'s handle of this job");
            if (hb.bytes != h->ipc_bytes || hb.layout != ipc_layout_word(h))
                throw Err("avae_comm_ipc_attach: rank " + std::to_string(r) + " was built with a different model / wire type / AVAE_IPC_BLOCKS");
            if (r == h->cfg.rank) continue;
            void* ptr = nullptr;
            if (hb.pid == (int32_t)getpid()) ptr = reinterpret_cast<void*>(hb.raw_ptr);          // a replica of this very process: its pointer is ours
            else { HIP_OK(hipIpcOpenMemHandle(&ptr, hb.mem, hipIpcMemLazyEnablePeerAccess)); h->ipc_opened[r] = true; }
            h->ipc_peer[r] = reinterpret_cast<unsigned char*>(ptr);
            h->ipc_args.peer[r] = h->ipc_peer[r];
        }
        h->ipc_attached = true;
    });
}

int avae_cost_history(avae_handle* h, int32_t n, float* host_dst, int64_t* last_step) {
    return guarded(h, [&] {
        if (n < 0 || n > kCostHist) throw Err("cost history request out of range");
        HIP_OK(hipDeviceSynchronize());
        comm_check_error(h);
        std::vector<unsigned char> buf(sizeof(DevState));
        HIP_OK(hipMemcpy(buf.data(), h->state(), sizeof(DevState), hipMemcpyDeviceToHost));
        const DevState* st = reinterpret_cast<const DevState*>(buf.data());
        if (st->step < n) throw Err("fewer steps applied than requested");
        for (int i = 0; i < n; ++i) host_dst[i] = st->cost_hist[(st->step - n + i) % kCostHist];
        if (last_step) *last_step = st->step;
    });
}

int avae_eval_cost(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, const float* eps_dev, float* cost_host, void* stream) {
    return guarded(h, [&] { eval_cost(h, h->plain, x_dev, x_ld, nullptr, nullptr, nullptr, eps_dev, cost_host, on_stream(h, stream)); });
}

int avae_encode(avae_handle* h, int32_t m, const float* x_dev, int32_t x_ld, int32_t rows, float* mu_dev, float* logvar_dev, void* stream) {
    return guarded(h, [&] {
        if (m < 0 || m >= h->M) throw Err("modality index out of range");
        if (rows < 0) throw Err("rows must be >= 0");
        hipStream_t s = on_stream(h, stream);
        const Mod& md = h->mods[m];
        const int ld = x_ld > 0 ? x_ld : md.n_in;
        const size_t nzb = (size_t)h->nz * 4;
        for (int r0 = 0; r0 < rows; r0 += h->B) {
            const int n = std::min(h->B, rows - r0);
            run_prep_single(h, PrepOne(x_dev + (size_t)r0 * ld, ld, n, md.n_in, md.X0).with_eps(nullptr, 0x656e63ull), s);
            run_inference(h, m, true, n, s);
            if (mu_dev) copy_rows(mu_dev + (size_t)r0 * h->nz, nzb, h->at<float>(md.mulv), 2 * nzb, nzb, n, s);
            if (logvar_dev) copy_rows(logvar_dev + (size_t)r0 * h->nz, nzb, h->at<float>(md.mulv) + h->nz, 2 * nzb, nzb, n, s);
        }
    });
}

int avae_decode(avae_handle* h, int32_t m, const float* z_dev, int32_t rows, float* xhat_dev, void* stream) {
    return guarded(h, [&] {
        if (m < 0 || m >= h->M) throw Err("modality index out of range");
        if (rows < 0) throw Err("rows must be >= 0");
        decode_rows(h, m, z_dev, rows, xhat_dev, on_stream(h, stream));
    });
}

int avae_generate(avae_handle* h, const float* z_dev, int32_t rows, float* const* xhat_dev, void* stream) {
    return guarded(h, [&] {
        if (rows < 0) throw Err("rows must be >= 0");
        if (!z_dev || !xhat_dev) throw Err("null argument");
        hipStream_t s = on_stream(h, stream);
        DecodeAll(h).run(rows, z_dev, true, xhat_dev, false, s);
    });
}

int avae_reconstruct(avae_handle* h, int32_t m, const float* x_dev, int32_t x_ld, const float* eps_dev, int32_t rows, float* xhat_dev, void* stream) {
    return guarded(h, [&] {
        if (m < 0 || m >= h->M) throw Err("modality index out of range");
        if (rows < 0) throw Err("rows must be >= 0");
        hipStream_t s = on_stream(h, stream);
        const Mod& md = h->mods[m];
        const int ld = x_ld > 0 ? x_ld : md.n_in;
        // a fresh eps per call and per modality (vae_assoc.py:423-424): the salt's high word carries (draw counter, modality), the
        // generator's row index is the row of the whole input (r0 + row)
        const unsigned long long draw = eps_dev ? 0ull : ((unsigned long long)next_draw(h, eps_dev) << 34) | ((unsigned long long)m << 32);
        for (int r0 = 0; r0 < rows; r0 += h->B) {
            const int n = std::min(h->B, rows - r0);
            run_prep_single(h, PrepOne(x_dev + (size_t)r0 * ld, ld, n, md.n_in, md.X0, r0)
                                   .with_eps(eps_dev ? eps_dev + (size_t)r0 * h->nz : nullptr, 0x7265636full | draw), s);
            run_inference(h, m, true, n, s);
            run_inference(h, m, false, n, s);
            copy_out32(h, m, xhat_dev + (size_t)r0 * md.n_in, n, s);
        }
    });
}

int avae_score_width(const avae_config* cfg, int32_t flags, int32_t* k) {
    try {
        if (!cfg || !k) throw Err("null argument");
        check_config(*cfg);
        if (flags & ~AVAE_SCORE_CROSS) throw Err("avae_score: unknown flags (only AVAE_SCORE_CROSS is defined)");
        const int M = cfg->n_modalities;
        *k = 1 + 2 * M + M * (M - 1) / 2 + ((flags & AVAE_SCORE_CROSS) ? M * M : 0);
        return 0;
    } catch (const std::exception& e) { g_create_error = e.what(); return 2; }
}

// Per chunk of at most batch_size rows: stage every modality (and eps) -> encoders -> k_score_latent (latent, assoc, z of every
// modality) -> per modality decoder + k_score_rows (the last one also forms cost); with AVAE_SCORE_CROSS then per source s:
// k_score_latent(z = mu_s) -> every decoder + k_score_rows.  The kernels write straight into the caller's score rows.
// present (avae_score_masked): the caller's [rows][M] presence bytes.  Staging copies each chunk's bytes (0 / 1, NULL sources folded
// in) into row_pres, which the MASK kernel instances read; every launch of the unmasked call is kept, absent rows run as zeros
// whose results the kernels select away.
static void score_call(avae_handle* h, const char* what, const float* const* x_dev, const int32_t* x_ld, const uint8_t* present,
                int32_t rows, const float* eps_dev, int32_t flags, float* out_dev, void* stream) {
        const std::string w = what;
        if (flags & ~AVAE_SCORE_CROSS) throw Err(w + ": unknown flags (only AVAE_SCORE_CROSS is defined)");
        if (rows < 0) throw Err(w + ": rows must be >= 0");
        if (rows == 0) return;
        if (!out_dev) throw Err(w + ": out_dev is NULL");
        if (!x_dev) throw Err(w + ": x_dev is NULL");
        const RowInputs in(h, w, x_dev, x_ld, present ? NullRows::Absent : NullRows::Required);
        const RowPresence pres = row_presence(h, present);
        const int M = h->M, P = M * (M - 1) / 2;
        const bool cross = (flags & AVAE_SCORE_CROSS) != 0;
        const int k = 1 + 2 * M + P + (cross ? M * M : 0);
        hipStream_t s = on_stream(h, stream);
        // a fresh eps per call, keyed as avae_reconstruct's: draw counter in the salt's high bits, row of the whole input
        const StageEps eps{eps_dev, 0x73636f72ull /*scor*/ | (unsigned long long)next_draw(h, eps_dev) << 34};
        ScoreLatentArgs la;
        std::memset(&la, 0, sizeof(la));
        la.eps = h->at<float>(h->off_eps); la.ld_eps = h->ld_eps;
        la.k = k; la.nz = h->nz; la.n_mod = M;
        ScoreRowsArgs ra;
        std::memset(&ra, 0, sizeof(ra));
        ra.k = k; ra.n_mod = M; ra.n_pair = P; ra.lambda = h->cfg.assoc_lambda;
        la.present = ra.present = pres.staged;
        for (int m = 0; m < M; ++m) {
            la.mulv[m] = h->at<float>(h->mods[m].mulv);
            la.Z[m] = h->at<void>(h->mods[m].Z.rm); la.ldz[m] = h->mods[m].Z.ld;
            ra.w[m] = h->cfg.mod[m].weight;
        }
        auto score_latent = [&](int src) {
            la.src = src;
            timed_launch(h, s, "score_latent", [&] { launch_score_latent(h->cfg.compute_dtype, la, s); });
        };
        // decoder m on the z in place, then its rows' terms into column col (src >= 0: cross term of source src)
        auto score_rows = [&](int m, int r0, int col, bool with_cost, int n, int src = -1) {
            const Mod& md = h->mods[m];
            run_inference(h, m, false, n, s);
            ra.x = in.at(m, r0); ra.ldx = in.ld[m];
            ra.pa = src < 0 ? m : src; ra.pb = m; ra.absent_bits = src < 0 ? 0u : 0x7FC00000u;      // (masked) +0.0 / quiet NaN
            ra.xhat = h->at<float>(md.out32); ra.ld32 = md.ld32;
            ra.n_in = md.n_in; ra.binary = h->cfg.mod[m].binary ? 1 : 0;
            ra.col = col; ra.cost = with_cost ? 1 : 0; ra.rows = n;
            timed_launch(h, s, "score_rows", [&] { launch_score_rows(ra, s); });
        };
        for (int r0 = 0; r0 < rows; r0 += h->B) {
            const int n = std::min(h->B, rows - r0);
            stage_and_encode(h, in, pres, r0, n, true, &eps, s);
            la.out = ra.out = out_dev + (size_t)r0 * k; la.rows = n;
            score_latent(-1);
            for (int m = 0; m < M; ++m) score_rows(m, r0, 1 + m, m == M - 1, n);
            if (!cross) continue;
            for (int src = 0; src < M; ++src) {
                score_latent(src);
                for (int d = 0; d < M; ++d) score_rows(d, r0, 1 + 2 * M + P + src * M + d, false, n, src);
            }
        }
}

int avae_score(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, int32_t rows, const float* eps_dev, int32_t flags,
               float* out_dev, void* stream) {
    return guarded(h, [&] { score_call(h, "avae_score", x_dev, x_ld, nullptr, rows, eps_dev, flags, out_dev, stream); });
}

int avae_score_masked(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, const uint8_t* present_dev, int32_t rows,
                      const float* eps_dev, int32_t flags, float* out_dev, void* stream) {
    return guarded(h, [&] {
        if (!present_dev) throw Err("avae_score_masked: present_dev is NULL (avae_score is the unmasked call)");
        score_call(h, "avae_score_masked", x_dev, x_ld, present_dev, rows, eps_dev, flags, out_dev, stream);
    });
}

// Importance-weighted log-likelihoods.  Passes of at most batch_size decoded rows (SampleBlocks).  Per chunk of n_rows input rows:
// stage + encode every modality once; per sample block and proposal src: k_iw_latent (z, r) -> every decoder (DecodeAll) ->
// k_iw_rows (log-weights) -> k_iw_reduce (running log-sum-exp; the row's last block writes the caller's row).  Scratch: iw_buf
// and the decoders' out32 / Z buffers.
// present (avae_loglik_masked): as score_call's.
static void loglik_call(avae_handle* h, const char* what, const float* const* x_dev, const int32_t* x_ld, const uint8_t* present,
                 int32_t rows, int32_t n_samples, const float* eps_dev, float* out_dev, void* stream) {
        const std::string w = what;
        if (rows < 0) throw Err(w + ": rows must be >= 0");
        if (n_samples < 1) throw Err(w + ": n_samples must be >= 1, got " + std::to_string(n_samples));
        if (rows == 0) return;
        if (!out_dev) throw Err(w + ": out_dev is NULL");
        if (!x_dev) throw Err(w + ": x_dev is NULL");
        const RowInputs in(h, w, x_dev, x_ld, present ? NullRows::Absent : NullRows::Required);
        const RowPresence pres = row_presence(h, present);
        const int M = h->M, B = h->B, nz = h->nz, K = n_samples;
        hipStream_t s = on_stream(h, stream);
        const int width = 2 * M + M * M;
        const SampleBlocks blocks(K, B);
        const size_t z_n = (size_t)B * nz, r_n = (size_t)B, ell_n = (size_t)B * M, st_n = (size_t)B * M * (2 + M) * 2;
        float* z32 = static_cast<float*>(h->iw_buf.ensure((z_n + r_n + ell_n + st_n) * sizeof(float)));
        float* rbuf = z32 + z_n;
        float* ell = rbuf + r_n;
        float* state = ell + ell_n;
        const DecodeAll dec(h);
        IwLatentArgs la;
        std::memset(&la, 0, sizeof(la));
        // a fresh eps per call, keyed as avae_score's: draw counter, row of the whole input (+ the sample index)
        la.nz = nz; la.K = K; la.seed = h->cfg.seed; la.draw = next_draw(h, eps_dev); la.r = rbuf; la.pres_ld = M;
        dec.z_dest(la, z32);
        IwRowsArgs ra;
        std::memset(&ra, 0, sizeof(ra));
        ra.ell = ell; ra.n_mod = M; ra.present = pres.staged;
        for (int m = 0; m < M; ++m) {
            const Mod& md = h->mods[m];
            ra.xhat[m] = h->at<float>(md.out32); ra.ldh[m] = dec.ld_out32(m);
            ra.n_in[m] = md.n_in; ra.binary[m] = h->cfg.mod[m].binary ? 1 : 0; ra.ldx[m] = in.ld[m];
        }
        IwReduceArgs rd;
        std::memset(&rd, 0, sizeof(rd));
        rd.ell = ell; rd.r = rbuf; rd.state = state; rd.width = width; rd.n_mod = M; rd.log_k = std::log((float)K); rd.present = pres.staged;
        for (int r0 = 0; r0 < rows; r0 += blocks.n_rows) {
            const int n = std::min(blocks.n_rows, rows - r0);
            stage_and_encode(h, in, pres, r0, n, true, nullptr, s);
            for (int m = 0; m < M; ++m) ra.x[m] = in.at(m, r0);
            la.eps = eps_dev ? eps_dev + (size_t)r0 * K * nz : nullptr;
            la.row0 = (long long)h->cfg.row_offset + r0;
            rd.out = out_dev + (size_t)r0 * width;
            la.rows = rd.rows = n;
            blocks.each(n, [&](int k0, int kc, int nd) {
                la.k0 = k0; la.kc = ra.kc = rd.kc = kc; ra.n_dec = nd;
                rd.first = k0 == 0; rd.last = k0 + kc == K;
                for (int src = 0; src < M; ++src) {
                    la.mulv = h->at<float>(h->mods[src].mulv);
                    la.present = pres ? pres.staged + src : nullptr;
                    timed_launch(h, s, "iw_latent", [&] { launch_iw_latent(h->cfg.compute_dtype, la, s); });
                    dec.run(nd, z32, false, nullptr, false, s);
                    timed_launch(h, s, "iw_rows", [&] { launch_iw_rows(ra, s); });
                    rd.src = src;
                    timed_launch(h, s, "iw_reduce", [&] { launch_iw_reduce(rd, s); });
                }
            });
        }
}

int avae_loglik(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, int32_t rows, int32_t n_samples,
                const float* eps_dev, float* out_dev, void* stream) {
    return guarded(h, [&] { loglik_call(h, "avae_loglik", x_dev, x_ld, nullptr, rows, n_samples, eps_dev, out_dev, stream); });
}

int avae_loglik_masked(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, const uint8_t* present_dev, int32_t rows,
                       int32_t n_samples, const float* eps_dev, float* out_dev, void* stream) {
    return guarded(h, [&] {
        if (!present_dev) throw Err("avae_loglik_masked: present_dev is NULL (avae_loglik is the unmasked call)");
        loglik_call(h, "avae_loglik_masked", x_dev, x_ld, present_dev, rows, n_samples, eps_dev, out_dev, stream);
    });
}

// Fused-posterior prediction of every modality from the ones a row has (include/avae.h).  Per chunk of at
// most batch_size rows: stage + encode every given modality once (a NULL x_dev[m] runs no encoder) -> k_impute_fuse ([mu_f | lv_f]
// into the scratch and the caller's rows; n_samples = 0: mu_f as the decoders' z, decoded once).  Then loglik_call's layout over
// the chunk's rows with `cap` decoded rows per group (SampleBlocks): per group the UNMASKED k_iw_latent on the fused rows (its r
// goes to scratch and is not read) -> the decoders (DecodeAll) -> k_impute_accum.  Modality by modality (conv nets / use_graph = 0
// / timing) a group is one pass, cap = batch_size, on the decoders' Z / out32 buffers; the serve route keeps up to P passes of z
// and outputs in the scratch, so the two row kernels run once per P decoder passes.  Scratch: imp_buf.
constexpr int kImputeGroupPasses = 16;                 // passes per group of the serve route, at most ...
constexpr size_t kImputeGroupBytes = (size_t)16 << 20;  // ... and at most this many bytes of decoder outputs held per group
static void impute_call(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, const uint8_t* present, int32_t rows,
                        int32_t n_samples, const float* eps_dev, float* mu_dev, float* logvar_dev, float* const* mean_dev,
                        float* const* var_dev, void* stream) {
        const std::string w = "avae_impute";
        if (rows < 0) throw Err(w + ": rows must be >= 0");
        if (n_samples < 0) throw Err(w + ": n_samples must be >= 0, got " + std::to_string(n_samples));
        if (rows == 0) return;
        if (!x_dev) throw Err(w + ": x_dev is NULL");
        const int M = h->M, B = h->B, nz = h->nz, K = n_samples;
        const RowInputs in(h, w, x_dev, x_ld, NullRows::Absent);
        float* mean_out[kMaxMod] = {nullptr, nullptr, nullptr, nullptr};
        float* var_out[kMaxMod] = {nullptr, nullptr, nullptr, nullptr};
        bool decode = false;
        int n_all = 0;
        for (int m = 0; m < M; ++m) {
            mean_out[m] = mean_dev ? mean_dev[m] : nullptr;
            var_out[m] = (var_dev && K > 0) ? var_dev[m] : nullptr;
            decode = decode || mean_out[m] || var_out[m];
            n_all += h->mods[m].n_in;
        }
        const RowPresence pres = row_presence(h, present);
        hipStream_t s = on_stream(h, stream);
        // P = passes of one group of the serve route (z and outputs in the scratch, at most kImputeGroupBytes of outputs)
        const int P = (int)std::max<size_t>(1, std::min<size_t>(kImputeGroupPasses, kImputeGroupBytes / ((size_t)B * n_all * sizeof(float))));
        const size_t f_n = (size_t)B * 2 * nz, z_n = rup((size_t)P * B * nz, 2), r_n = rup((size_t)P * B, 2), st_n = (size_t)n_all * 2;
        const size_t o_n = P > 1 ? (size_t)P * B * n_all : 0;
        float* fused = static_cast<float*>(h->imp_buf.ensure((f_n + z_n + r_n + st_n + o_n) * sizeof(float)));
        float* z32 = fused + f_n;
        float* rbuf = z32 + z_n;
        float* state = rbuf + r_n;                 // (an even float offset: k_impute_accum moves float2)
        float* outs = state + st_n;
        const DecodeAll dec(h);
        const bool grouped = !dec.by_mod && P > 1;
        const int cap = grouped ? P * B : B;       // decoded rows of one group
        const SampleBlocks blocks(K, cap);         // input rows, samples of one group
        ImputeFuseArgs fa;
        std::memset(&fa, 0, sizeof(fa));
        fa.mods = in.mods; fa.present = pres.staged; fa.fused = fused; fa.nz = nz; fa.n_mod = M;
        for (int m = 0; m < M; ++m) fa.mulv[m] = h->at<float>(h->mods[m].mulv);
        IwLatentArgs la;
        std::memset(&la, 0, sizeof(la));
        la.mulv = fused; la.nz = nz; la.K = K; la.seed = h->cfg.seed; la.r = rbuf; la.pres_ld = M;
        // a fresh eps per sampled call, keyed as avae_loglik's: draw counter, row of the whole input, sample index
        if (K > 0 && decode) la.draw = next_draw(h, eps_dev);
        if (decode) dec.z_dest(la, z32);
        if (decode && K == 0) dec.z_dest(fa, z32);  // the fuse launch stages z = mu_f itself
        ImputeAccumArgs aa;
        std::memset(&aa, 0, sizeof(aa));
        aa.state = state; aa.ld_state = n_all; aa.K = K; aa.n_mod = M;
        float* group_out[kMaxMod] = {nullptr, nullptr, nullptr, nullptr};     // grouped: the scratch rows the decoders store into
        for (int m = 0; m < M; ++m) {
            const Mod& md = h->mods[m];
            aa.col0[m] = m ? aa.col0[m - 1] + h->mods[m - 1].n_in : 0;
            if (grouped) group_out[m] = outs + (size_t)cap * aa.col0[m];
            aa.xhat[m] = grouped ? group_out[m] : h->at<float>(md.out32);
            aa.ldh[m] = dec.ld_out32(m);
            aa.n_in[m] = md.n_in;
            aa.tile0[m + 1] = aa.tile0[m] + (md.n_in + 63) / 64;
        }
        for (int r0 = 0; r0 < rows; r0 += B) {
            const int n = std::min(B, rows - r0);
            stage_and_encode(h, in, pres, r0, n, false, nullptr, s);
            fa.rows = n;
            fa.mu = mu_dev ? mu_dev + (size_t)r0 * nz : nullptr;
            fa.lv = logvar_dev ? logvar_dev + (size_t)r0 * nz : nullptr;
            timed_launch(h, s, "impute_fuse", [&] { launch_impute_fuse(h->cfg.compute_dtype, fa, s); });
            if (!decode) continue;
            if (K == 0) {                          // as avae_generate: the rows go straight to the caller (the decoders asked for)
                float* dst[kMaxMod] = {nullptr, nullptr, nullptr, nullptr};
                for (int d = 0; d < M; ++d) dst[d] = mean_out[d] ? mean_out[d] + (size_t)r0 * h->mods[d].n_in : nullptr;
                dec.run(n, z32, false, dst, true, s);
                continue;
            }
            for (int j0 = 0; j0 < n; j0 += blocks.n_rows) {    // the sample groups of this chunk's rows [j0, j0 + nj)
                const int nj = std::min(blocks.n_rows, n - j0), q0 = r0 + j0;
                la.mulv = fused + (size_t)j0 * 2 * nz;
                la.eps = eps_dev ? eps_dev + (size_t)q0 * K * nz : nullptr;
                la.row0 = (long long)h->cfg.row_offset + q0;
                la.rows = aa.rows = nj;
                for (int m = 0; m < M; ++m) {
                    aa.mean[m] = mean_out[m] ? mean_out[m] + (size_t)q0 * h->mods[m].n_in : nullptr;
                    aa.var[m] = var_out[m] ? var_out[m] + (size_t)q0 * h->mods[m].n_in : nullptr;
                }
                blocks.each(nj, [&](int k0, int kc, int nd) {
                    la.k0 = aa.k0 = k0; la.kc = aa.kc = kc;
                    timed_launch(h, s, "impute_latent", [&] { launch_iw_latent(h->cfg.compute_dtype, la, s); });
                    dec.run(nd, z32, false, grouped ? group_out : nullptr, false, s);     // (rows are independent: any pass split)
                    timed_launch(h, s, "impute_accum", [&] { launch_impute_accum(aa, s); });
                });
            }
        }
}

int avae_impute(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, const uint8_t* present_dev, int32_t rows,
                int32_t n_samples, const float* eps_dev, float* mu_dev, float* logvar_dev, float* const* mean_dev,
                float* const* var_dev, void* stream) {
    return guarded(h, [&] {
        impute_call(h, x_dev, x_ld, present_dev, rows, n_samples, eps_dev, mu_dev, logvar_dev, mean_dev, var_dev, stream);
    });
}

int avae_complete(avae_handle* h, const float* const* x_dev, const int32_t* x_ld, const uint8_t* const* obs_dev,
                  const float* z0_dev, int32_t rows, int32_t n_iters, float lr, float prior_weight,
                  float* z_dev, float* obj_dev, float* grad_dev, float* const* xhat_dev, void* stream) {
    return guarded(h, [&] {
        if (rows < 0) throw Err("avae_complete: rows must be >= 0");
        if (n_iters < 0) throw Err("avae_complete: n_iters must be >= 0, got " + std::to_string(n_iters));
        for (const Mod& md : h->mods)
            if (md.conv) throw Err("avae_complete: MLP decoders only (this model has a conv modality)");
        if (rows == 0) return;
        if (!x_dev) throw Err("avae_complete: x_dev is NULL");
        if (!z0_dev) throw Err("avae_complete: z0_dev is NULL");
        if (!z_dev) throw Err("avae_complete: z_dev is NULL");
        const int M = h->M, nz = h->nz;
        const RowInputs in(h, "avae_complete", x_dev, x_ld, NullRows::Unobserved);
        hipStream_t s = on_stream(h, stream);
        avae_handle::Complete& cp = complete_plan(h);
        const bool graphs = h->cfg.use_graph && !h->timing;
        for (int r0 = 0; r0 < rows; r0 += h->B) {
            CompleteCall c;
            std::memset(&c, 0, sizeof(c));
            for (int m = 0; m < M; ++m) {
                const size_t n_in = (size_t)h->mods[m].n_in;
                if (in.x[m]) {
                    c.x[m] = in.at(m, r0); c.ldx[m] = in.ld[m];
                    if (obs_dev && obs_dev[m]) c.obs[m] = obs_dev[m] + (size_t)r0 * n_in;
                }
                if (xhat_dev && xhat_dev[m]) c.xhat[m] = xhat_dev[m] + (size_t)r0 * n_in;
            }
            c.z0 = z0_dev + (size_t)r0 * nz; c.z_out = z_dev + (size_t)r0 * nz;
            c.obj = obj_dev ? obj_dev + r0 : nullptr; c.obj_ld = rows;
            c.grad = grad_dev ? grad_dev + (size_t)r0 * nz : nullptr;
            c.rows = std::min(h->B, rows - r0); c.n_iters = n_iters; c.lr = lr; c.prior = prior_weight;
            timed_launch(h, s, "complete_begin", [&] { launch_complete_begin(h->cfg.compute_dtype, cp.args, c, s); });
            int left = n_iters + 1;              // n_iters updating passes and the evaluation at the final z
            if (graphs)
                for (int i = 0; i < 3; ++i)
                    for (; left >= kCompleteSizes[i]; left -= kCompleteSizes[i]) HIP_OK(hipGraphLaunch(cp.g[i].exec, s));
            for (; left > 0; --left) complete_pass(h, cp, s);
        }
    });
}

// ---- cross-modal retrieval (include/avae.h, avae_retrieve.h)
static void check_topk_shape(const std::string& w, int32_t rows, int32_t gallery_rows, int32_t k) {
    if (k < 1 || k > AVAE_TOPK_MAX)
        throw Err(w + ": k = " + std::to_string(k) + " must be in [1, " + std::to_string(AVAE_TOPK_MAX) + "] (AVAE_TOPK_MAX)");
    check_rows(w, rows, "rows");
    check_rows(w, gallery_rows, "gallery_rows");
}

int avae_latent_topk_plan(const avae_config* cfg, int32_t rows, int32_t gallery_rows, int32_t k, int32_t* query_tile,
                          int32_t* gallery_tile, int32_t* n_splits, size_t* scratch_bytes) {
    return plan_query(cfg, [&] {
        check_topk_shape("avae_latent_topk_plan", rows, gallery_rows, k);
        const TopkPlan p = topk_plan(rows, gallery_rows, k);
        put(query_tile, p.query_tile); put(gallery_tile, p.gallery_tile); put(n_splits, p.n_splits);
        put(scratch_bytes, p.scratch_bytes);
    });
}

int avae_latent_topk(avae_handle* h, const float* q_mu_dev, const float* q_logvar_dev, int32_t rows, const float* g_mu_dev,
                     const float* g_logvar_dev, int32_t gallery_rows, int32_t metric, int32_t k, int32_t* index_dev,
                     float* dist_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_latent_topk";
        check_topk_shape(w, rows, gallery_rows, k);
        const bool kl = check_metric(w, metric);
        if (rows > 0) need(w, q_mu_dev, "q_mu_dev");
        if (gallery_rows > 0) need(w, g_mu_dev, "g_mu_dev");
        if (kl && rows > 0) need(w, q_logvar_dev, "q_logvar_dev", kNeedsLogvar);
        if (kl && gallery_rows > 0) need(w, g_logvar_dev, "g_logvar_dev", kNeedsLogvar);
        if (rows == 0 || (!index_dev && !dist_dev)) return;
        static_assert(kTopkMaxNz >= 64, "check_config bounds n_z by 64");
        const int nz = h->nz;
        const TopkPlan p = topk_plan(rows, gallery_rows, k);
        hipStream_t s = on_stream(h, stream);
        TopkArgs a = zeroed<TopkArgs>();
        a.g_mu = g_mu_dev; a.g_lv = kl ? g_logvar_dev : nullptr;
        a.gallery_rows = gallery_rows; a.nz = nz; a.k = k; a.metric = metric;
        a.n_splits = p.n_splits; a.tiles_per_split = p.tiles_per_split;
        if (p.n_splits > 0) a.part = scratch_of<unsigned long long>(h->topk_buf, w, p.scratch_bytes, kTopkScratchBytes);
        for (int r0 = 0; r0 < rows; r0 += p.chunk_rows) {
            a.rows = std::min(p.chunk_rows, rows - r0);
            a.q_mu = q_mu_dev + (size_t)r0 * nz;
            a.q_lv = kl ? q_logvar_dev + (size_t)r0 * nz : nullptr;
            a.index = index_dev ? index_dev + (size_t)r0 * k : nullptr;
            a.dist = dist_dev ? dist_dev + (size_t)r0 * k : nullptr;
            if (p.n_splits > 0) timed_launch(h, s, "latent_topk", [&] { launch_latent_topk(a, s); });
            timed_launch(h, s, "latent_topk_merge", [&] { launch_latent_topk_merge(a, s); });
        }
    });
}

// ---- per-dimension posterior diagnostics (include/avae.h, avae_latent_stats.h)
int avae_latent_stats_plan(const avae_config* cfg, int32_t rows, int32_t* row_tile, int32_t* n_slices, size_t* scratch_bytes) {
    return plan_query(cfg, [&] {
        check_rows("avae_latent_stats_plan", rows, "rows");
        const StatsPlan p = stats_plan(rows);
        put(row_tile, p.row_tile); put(n_slices, p.n_slices);
        put(scratch_bytes, stats_scratch_bytes(p.n_slices, cfg->n_modalities, cfg->n_z));
    });
}

int avae_latent_stats(avae_handle* h, int32_t n_mod, const float* const* mu_dev, const float* const* logvar_dev,
                      const uint8_t* present_dev, int32_t rows, const avae_latent_stats_out* out, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_latent_stats";
        if (n_mod < 1 || n_mod > AVAE_MAX_MODALITIES)
            throw Err(w + ": n_mod = " + std::to_string(n_mod) + " must be in [1, " + std::to_string(AVAE_MAX_MODALITIES) + "] (AVAE_MAX_MODALITIES)");
        check_rows(w, rows, "rows");
        need(w, out, "out");
        need(w, mu_dev, "mu_dev", "the array of pointers; a NULL entry marks an absent modality");
        for (int m = 0; m < n_mod; ++m)
            if (mu_dev[m] && (!logvar_dev || !logvar_dev[m]))
                throw Err(w + ": logvar_dev[" + std::to_string(m) + "] is NULL while mu_dev[" + std::to_string(m) + "] is given");
        if (!out->count && !out->mean && !out->var && !out->xcov && !out->assoc && !out->post_var && !out->kl && !out->cov) return;
        static_assert(kStatsMaxNz >= 64 && kMaxMod == AVAE_MAX_MODALITIES, "check_config bounds n_z by 64");
        const StatsPlan p = stats_plan(rows);
        hipStream_t s = on_stream(h, stream);
        StatsArgs a = zeroed<StatsArgs>();
        for (int m = 0; m < n_mod; ++m) { a.mu[m] = mu_dev[m]; a.lv[m] = mu_dev[m] ? logvar_dev[m] : nullptr; }
        a.present = present_dev; a.rows = rows; a.n_mod = n_mod; a.nz = h->nz;
        a.n_slices = p.n_slices; a.row_tile = p.row_tile; a.want_cov = out->cov ? 1 : 0; a.out = *out;
        if (p.n_slices > 0) {
            a.scratch = scratch_of<double>(h->stats_buf, w, stats_scratch_bytes(p.n_slices, n_mod, h->nz), kStatsScratchBytes);
            timed_launch(h, s, "latent_stats", [&] { launch_latent_stats(a, s); });
        }
        timed_launch(h, s, "latent_stats_merge", [&] { launch_latent_stats_merge(a, s); });
    });
}

// ---- motion decoding (include/avae.h, avae_motion.h)
static void check_range(const std::string& w, const char* name, int v, int lo, int hi) {
    if (v < lo || v > hi)
        throw Err(w + ": " + name + " = " + std::to_string(v) + " must be in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
}

// "must be finite and > 0" (strict) / ">= 0" for a float or double option
static void check_finite(const std::string& w, const char* name, double v, bool strict) {
    if (!std::isfinite(v) || (strict ? !(v > 0.0) : v < 0.0)) throw Err(w + ": " + name + " must be finite and " + (strict ? "> 0" : ">= 0"));
}

static void check_motion_shape(const std::string& w, int32_t rows, int32_t D, int32_t Kb, int32_t T, int32_t nc) {
    check_rows(w, rows, "rows");
    check_range(w, "D", D, 1, kMotionMaxD);
    check_range(w, "Kb", Kb, 1, kMotionMaxKb);
    check_range(w, "T", T, 1, kMotionMaxT);
    check_range(w, "nc", nc, 0, kMotionMaxNc);
}

static MotionArgs motion_args(const std::string& w, const float* params, int32_t rows, int32_t S, int32_t D, int32_t Kb, int32_t T,
                              const float* phi, const float* scale, const float* shift, const float* limits, const float* gain,
                              const float* target, int32_t nc, bool moments) {
    check_motion_shape(w, rows, D, Kb, T, nc);
    if (S < 1) throw Err(w + ": S = " + std::to_string(S) + " must be >= 1");
    need(w, params, moments ? "samples_dev" : "params_dev");
    need(w, phi, "phi_dev");
    if (nc > 0 && !gain) throw Err(w + ": anchor_gain_dev is NULL with nc > 0");
    if (nc > 0 && !target) throw Err(w + ": anchor_target_dev is NULL with nc > 0");
    if (motion_lds_bytes(D, Kb, T, nc, moments, true) > kMotionMaxLds) throw Err("internal error: " + w + " plans more LDS than its bound");
    MotionArgs a = zeroed<MotionArgs>();
    a.params = params; a.phi = phi; a.scale = scale; a.shift = shift; a.limits = limits;
    a.gain = nc > 0 ? gain : nullptr; a.target = nc > 0 ? target : nullptr;
    a.rows = rows; a.S = S; a.D = D; a.Kb = Kb; a.T = T; a.nc = nc;
    return a;
}

int avae_motion_eval(avae_handle* h, const float* params_dev, int32_t rows, int32_t D, int32_t Kb, int32_t T,
                     const float* phi_dev, const float* scale_dev, const float* shift_dev, const float* limits_dev,
                     const float* anchor_gain_dev, const float* anchor_target_dev, int32_t nc,
                     const float* ref_traj_dev, const float* ref_params_dev,
                     float* traj_dev, int32_t* saturated_dev, float* rmse_dev, float* maxabs_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_motion_eval";
        MotionArgs a = motion_args(w, params_dev, rows, 1, D, Kb, T, phi_dev, scale_dev, shift_dev, limits_dev, anchor_gain_dev,
                                   anchor_target_dev, nc, false);
        if (ref_traj_dev && ref_params_dev) throw Err(w + ": ref_traj_dev and ref_params_dev are both given; pass one reference");
        if ((rmse_dev || maxabs_dev) && !ref_traj_dev && !ref_params_dev)
            throw Err(w + ": rmse_dev / maxabs_dev need a reference (ref_traj_dev or ref_params_dev)");
        if (!traj_dev && !saturated_dev && !rmse_dev && !maxabs_dev) throw Err(w + ": every output is NULL");
        if (rows == 0) return;
        a.ref_traj = ref_traj_dev; a.ref_params = ref_params_dev;
        a.traj = traj_dev; a.saturated = saturated_dev; a.rmse = rmse_dev; a.maxabs = maxabs_dev;
        if (!rmse_dev && !maxabs_dev) { a.ref_traj = nullptr; a.ref_params = nullptr; }      // (a reference nobody reads)
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "motion_eval", [&] { launch_motion_eval(a, s); });
    });
}

int avae_motion_fit(avae_handle* h, const float* traj_dev, int32_t rows, int32_t D, int32_t Kb, int32_t T,
                    const float* pinv_dev, const float* scale_dev, const float* shift_dev, float* params_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_motion_fit";
        check_motion_shape(w, rows, D, Kb, T, 0);
        need(w, traj_dev, "traj_dev"); need(w, pinv_dev, "pinv_dev"); need(w, params_dev, "params_dev");
        if (rows == 0) return;
        MotionFitArgs a = zeroed<MotionFitArgs>();
        a.traj = traj_dev; a.pinv = pinv_dev; a.scale = scale_dev; a.shift = shift_dev; a.params = params_dev;
        a.rows = rows; a.D = D; a.Kb = Kb; a.T = T;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "motion_fit", [&] { launch_motion_fit(a, s); });
    });
}

int avae_motion_moments(avae_handle* h, const float* samples_dev, int32_t rows, int32_t S, int32_t D, int32_t Kb, int32_t T,
                        const float* phi_dev, const float* scale_dev, const float* shift_dev, const float* limits_dev,
                        const float* anchor_gain_dev, const float* anchor_target_dev, int32_t nc,
                        float* mean_dev, float* var_dev, float* saturated_frac_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_motion_moments";
        MotionArgs a = motion_args(w, samples_dev, rows, S, D, Kb, T, phi_dev, scale_dev, shift_dev, limits_dev, anchor_gain_dev,
                                   anchor_target_dev, nc, true);
        need(w, mean_dev, "mean_dev");
        if (rows == 0) return;
        a.traj = mean_dev; a.var = var_dev; a.sat_frac = saturated_frac_dev;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "motion_moments", [&] { launch_motion_moments(a, s); });
    });
}

// ---- pen-path kinematics and stroke rendering (include/avae.h, avae_render.h)
int avae_motion_fk(avae_handle* h, const float* traj_dev, int32_t rows, int32_t T, int32_t D,
                   const float* frames_dev, const float* axes_dev, float* path_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_motion_fk";
        check_rows(w, rows, "rows");
        check_range(w, "T", T, 1, kRenderMaxT);
        check_range(w, "D", D, 1, kFkMaxD);
        need(w, traj_dev, "traj_dev"); need(w, frames_dev, "frames_dev"); need(w, axes_dev, "axes_dev"); need(w, path_dev, "path_dev");
        if (rows == 0) return;
        FkArgs a = zeroed<FkArgs>();
        a.traj = traj_dev; a.frames = frames_dev; a.axes = axes_dev; a.path = path_dev;
        a.points = (long long)rows * T; a.D = D;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "motion_fk", [&] { launch_motion_fk(a, s); });
    });
}

int avae_stroke_render(avae_handle* h, const float* path_dev, int32_t rows, int32_t T, const float* plane_dev,
                       float half_width, float margin, int32_t H, int32_t ss,
                       const float* target_dev, const float* height_dev,
                       float* image_dev, float* window_dev, float* img_l2_dev, float* height_l2_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_stroke_render";
        check_rows(w, rows, "rows");
        check_range(w, "T", T, 1, kRenderMaxT);
        check_range(w, "H", H, 1, kRenderMaxH);
        if (ss != 1 && ss != 2 && ss != 4 && ss != 8) throw Err(w + ": ss = " + std::to_string(ss) + " must be 1, 2, 4 or 8");
        check_finite(w, "half_width", half_width, true);
        check_finite(w, "margin", margin, false);
        need(w, path_dev, "path_dev"); need(w, plane_dev, "plane_dev");
        if (!image_dev && !window_dev && !img_l2_dev && !height_l2_dev) throw Err(w + ": every output is NULL");
        if (img_l2_dev && !target_dev) throw Err(w + ": img_l2_dev needs target_dev");
        if (height_l2_dev && !height_dev) throw Err(w + ": height_l2_dev needs height_dev");
        if (render_lds_bytes(T, H) > 65536) throw Err("internal error: " + w + " plans more LDS than its bound");
        if (rows == 0) return;
        RenderArgs a = zeroed<RenderArgs>();
        a.path = path_dev; a.plane = plane_dev; a.target = img_l2_dev ? target_dev : nullptr;       // (a target nobody reads)
        a.height = height_l2_dev ? height_dev : nullptr;
        a.image = image_dev; a.window = window_dev; a.img_l2 = img_l2_dev; a.height_l2 = height_l2_dev;
        a.half_width = half_width; a.margin = margin; a.T = T; a.H = H; a.ss = ss;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "stroke_render", [&] { launch_stroke_render(a, rows, s); });
    });
}

// ---- gradients through the writing chain (include/avae.h, avae_grad.h)
int avae_stroke_render_vjp(avae_handle* h, const float* path_dev, int32_t rows, int32_t T, const float* plane_dev,
                           float half_width, float margin, int32_t H, int32_t ss,
                           const float* target_dev, const float* height_dev,
                           const float* g_image_dev, const float* g_img_l2_dev, const float* g_height_l2_dev,
                           float* grad_path_dev, float* image_dev, float* window_dev, float* img_l2_dev, float* height_l2_dev,
                           float* objective_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_stroke_render_vjp";
        check_rows(w, rows, "rows");
        check_range(w, "T", T, 1, kRenderMaxT);
        check_range(w, "H", H, 1, kRenderMaxH);
        if (ss != 1 && ss != 2 && ss != 4 && ss != 8) throw Err(w + ": ss = " + std::to_string(ss) + " must be 1, 2, 4 or 8");
        check_finite(w, "half_width", half_width, true);
        check_finite(w, "margin", margin, false);
        need(w, path_dev, "path_dev"); need(w, plane_dev, "plane_dev"); need(w, grad_path_dev, "grad_path_dev");
        if ((img_l2_dev || g_img_l2_dev) && !target_dev) throw Err(w + ": img_l2_dev and g_img_l2_dev need target_dev");
        if ((height_l2_dev || g_height_l2_dev) && !height_dev) throw Err(w + ": height_l2_dev and g_height_l2_dev need height_dev");
        if (render_vjp_lds_bytes(T, H) > kMaxDynLds) throw Err("internal error: " + w + " plans more LDS than its bound");
        if (rows == 0) return;
        RenderVjpArgs a = zeroed<RenderVjpArgs>();
        a.f.path = path_dev; a.f.plane = plane_dev; a.f.target = (img_l2_dev || g_img_l2_dev) ? target_dev : nullptr;
        a.f.height = (height_l2_dev || g_height_l2_dev) ? height_dev : nullptr;
        a.f.image = image_dev; a.f.window = window_dev; a.f.img_l2 = img_l2_dev; a.f.height_l2 = height_l2_dev;
        a.f.half_width = half_width; a.f.margin = margin; a.f.T = T; a.f.H = H; a.f.ss = ss;
        a.g_image = g_image_dev; a.g_img_l2 = g_img_l2_dev; a.g_height_l2 = g_height_l2_dev;
        a.grad_path = grad_path_dev; a.objective = objective_dev;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "stroke_render_vjp", [&] { launch_stroke_render_vjp(a, rows, s); });
    });
}

int avae_motion_fk_vjp(avae_handle* h, const float* traj_dev, int32_t rows, int32_t T, int32_t D,
                       const float* frames_dev, const float* axes_dev, const float* grad_path_dev, float* grad_traj_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_motion_fk_vjp";
        check_rows(w, rows, "rows");
        check_range(w, "T", T, 1, kRenderMaxT);
        check_range(w, "D", D, 1, kFkMaxD);
        need(w, traj_dev, "traj_dev"); need(w, frames_dev, "frames_dev"); need(w, axes_dev, "axes_dev");
        need(w, grad_path_dev, "grad_path_dev"); need(w, grad_traj_dev, "grad_traj_dev");
        if (rows == 0) return;
        FkVjpArgs a = zeroed<FkVjpArgs>();
        a.traj = traj_dev; a.frames = frames_dev; a.axes = axes_dev; a.grad_path = grad_path_dev; a.grad_traj = grad_traj_dev;
        a.points = (long long)rows * T; a.D = D;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "motion_fk_vjp", [&] { launch_motion_fk_vjp(a, s); });
    });
}

int avae_motion_eval_vjp(avae_handle* h, const float* params_dev, int32_t rows, int32_t D, int32_t Kb, int32_t T,
                         const float* phi_dev, const float* scale_dev, const float* shift_dev, const float* limits_dev,
                         const float* anchor_gain_dev, const float* anchor_target_dev, int32_t nc,
                         const float* grad_traj_dev, float* grad_params_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_motion_eval_vjp";
        check_motion_shape(w, rows, D, Kb, T, nc);
        need(w, params_dev, "params_dev"); need(w, phi_dev, "phi_dev");
        need(w, grad_traj_dev, "grad_traj_dev"); need(w, grad_params_dev, "grad_params_dev");
        if (nc > 0 && !anchor_gain_dev) throw Err(w + ": anchor_gain_dev is NULL with nc > 0");
        if (nc > 0 && !anchor_target_dev) throw Err(w + ": anchor_target_dev is NULL with nc > 0");
        if (rows == 0) return;
        static_assert(kFitSlab * kMotionMaxNc <= 1024 && kMotionMaxD * kMotionMaxKb % kMotionThreads == 0, "k_motion_eval_vjp's tiles");
        MotionVjpArgs a = zeroed<MotionVjpArgs>();
        a.params = params_dev; a.phi = phi_dev; a.scale = scale_dev; a.shift = shift_dev; a.limits = limits_dev;
        a.gain = nc > 0 ? anchor_gain_dev : nullptr; a.target = nc > 0 ? anchor_target_dev : nullptr;
        a.grad_traj = grad_traj_dev; a.grad_params = grad_params_dev;
        a.rows = rows; a.D = D; a.Kb = Kb; a.T = T; a.nc = nc;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "motion_eval_vjp", [&] { launch_motion_eval_vjp(a, s); });
    });
}

int avae_rows_adam(avae_handle* h, float* x_dev, const float* g_dev, float* m_dev, float* v_dev, int32_t* t_dev, int32_t* status_dev,
                   int32_t P, int32_t n, float lr, float beta1, float beta2, float eps, float max_norm,
                   const float* cost_dev, float* best_cost_dev, float* best_x_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_rows_adam";
        check_rows(w, P, "P");
        check_range(w, "n", n, 1, kRowsAdamMaxN);
        check_finite(w, "lr", lr, false);
        check_finite(w, "eps", eps, true);
        if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f)) throw Err(w + ": beta1 and beta2 must be in [0, 1)");
        if (std::isnan(max_norm)) throw Err(w + ": max_norm must not be NaN (<= 0: no clipping)");
        need(w, x_dev, "x_dev"); need(w, g_dev, "g_dev"); need(w, m_dev, "m_dev"); need(w, v_dev, "v_dev");
        need(w, t_dev, "t_dev"); need(w, status_dev, "status_dev");
        if (cost_dev && (!best_cost_dev || !best_x_dev)) throw Err(w + ": cost_dev needs best_cost_dev and best_x_dev");
        if (P == 0) return;
        RowsAdamArgs a = zeroed<RowsAdamArgs>();
        a.x = x_dev; a.g = g_dev; a.m = m_dev; a.v = v_dev; a.t = t_dev; a.status = status_dev;
        a.cost = cost_dev; a.best_cost = cost_dev ? best_cost_dev : nullptr; a.best_x = cost_dev ? best_x_dev : nullptr;
        a.n = n; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.max_norm = max_norm;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "rows_adam", [&] { launch_rows_adam(a, P, s); });
    });
}

// ---- letter thumbnails (include/avae.h, avae_thumbnail.h)
static void check_thumb_frame(const std::string& w, int32_t rows, int32_t Hf, int32_t Wf) {
    check_rows(w, rows, "rows");
    if (rows > kThumbMaxRows) throw Err(w + ": rows = " + std::to_string(rows) + " must be at most " + std::to_string(kThumbMaxRows));
    check_range(w, "Hf", Hf, 1, kThumbMaxFrame);
    check_range(w, "Wf", Wf, 1, kThumbMaxFrame);
}

int avae_letter_thumbnail_plan(int32_t rows, int32_t Hf, int32_t Wf, int32_t* slabs, size_t* workspace_bytes) {
    try {
        const std::string w = "avae_letter_thumbnail_plan";
        check_thumb_frame(w, rows, Hf, Wf);
        if (!slabs && !workspace_bytes) throw Err(w + ": every output is NULL");
        const ThumbPlan p = thumb_plan(Hf, Wf);
        if (slabs) *slabs = p.slabs;
        if (workspace_bytes) *workspace_bytes = thumb_workspace_bytes(rows, p.slabs);
        return 0;
    } catch (const std::exception& e) { g_create_error = e.what(); return 2; }
}

int avae_letter_thumbnail(avae_handle* h, const uint8_t* frames_dev, int32_t rows, int32_t Hf, int32_t Wf, int32_t C,
                          int64_t row_stride, int64_t frame_stride, int32_t flags, int32_t threshold, int32_t size,
                          void* workspace_dev, size_t workspace_bytes,
                          float* image_dev, int32_t* box_dev, int32_t* window_dev, int32_t* ink_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_letter_thumbnail";
        check_thumb_frame(w, rows, Hf, Wf);
        if (C != 1 && C != 3 && C != 4) throw Err(w + ": C = " + std::to_string(C) + " must be 1, 3 or 4");
        check_range(w, "size", size, 1, kThumbMaxSize);
        check_range(w, "threshold", threshold, -1, 255);
        if (flags & ~(AVAE_THUMB_INVERT | AVAE_THUMB_BGR))
            throw Err(w + ": flags = " + std::to_string(flags) + " holds bits other than AVAE_THUMB_INVERT | AVAE_THUMB_BGR");
        const long long row_bytes = (long long)Wf * C;
        if (row_stride < row_bytes || row_stride > kThumbMaxRowStride)
            throw Err(w + ": row_stride = " + std::to_string(row_stride) + " must be in [Wf * C = " + std::to_string(row_bytes) + ", " +
                      std::to_string(kThumbMaxRowStride) + "]");
        const long long frame_bytes = (long long)(Hf - 1) * row_stride + row_bytes;      // (row_stride <= 2^26: below 2^38)
        if (frame_stride < frame_bytes || frame_stride > kThumbMaxFrameStride)
            throw Err(w + ": frame_stride = " + std::to_string(frame_stride) + " must be in [(Hf - 1) * row_stride + Wf * C = " +
                      std::to_string(frame_bytes) + ", " + std::to_string(kThumbMaxFrameStride) + "]");
        need(w, frames_dev, "frames_dev");
        if (!image_dev && !box_dev && !window_dev && !ink_dev) throw Err(w + ": every output is NULL");
        if (rows == 0) return;
        const ThumbPlan p = thumb_plan(Hf, Wf);
        const size_t want = thumb_workspace_bytes(rows, p.slabs);
        need(w, workspace_dev, "workspace_dev");
        if (workspace_bytes < want)
            throw Err(w + ": workspace_bytes = " + std::to_string(workspace_bytes) + " is below the " + std::to_string(want) +
                      " bytes avae_letter_thumbnail_plan gives");
        if (reinterpret_cast<uintptr_t>(workspace_dev) % 16 != 0) throw Err(w + ": workspace_dev must be aligned to 16 bytes");
        ThumbArgs a = zeroed<ThumbArgs>();
        a.frames = frames_dev; a.row_stride = row_stride; a.frame_stride = frame_stride;
        a.records = static_cast<int32_t*>(workspace_dev);
        a.image = image_dev; a.box = box_dev; a.window = window_dev; a.ink = ink_dev;
        a.Hf = Hf; a.Wf = Wf; a.C = C;
        a.invert = (flags & AVAE_THUMB_INVERT) ? 1 : 0; a.bgr = (flags & AVAE_THUMB_BGR) ? 1 : 0; a.threshold = threshold;
        a.size = size; a.slab_rows = p.slab_rows; a.slabs = p.slabs;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "ink_box", [&] { launch_ink_box(a, rows, s); });
        timed_launch(h, s, "thumbnail", [&] { launch_thumbnail(a, rows, s); });
    });
}

// ---- pose, Jacobian and inverse kinematics (include/avae.h, avae_ik.h)
int avae_motion_pose(avae_handle* h, const float* traj_dev, int32_t rows, int32_t T, int32_t D,
                     const float* frames_dev, const float* axes_dev,
                     float* position_dev, float* rotation_dev, float* jacobian_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_motion_pose";
        check_rows(w, rows, "rows");
        check_range(w, "T", T, 1, kIkMaxT);
        check_range(w, "D", D, 1, kIkMaxD);
        need(w, traj_dev, "traj_dev"); need(w, frames_dev, "frames_dev"); need(w, axes_dev, "axes_dev");
        if (!position_dev && !rotation_dev && !jacobian_dev) throw Err(w + ": every output is NULL");
        if (rows == 0) return;
        PoseArgs a = zeroed<PoseArgs>();
        a.traj = traj_dev; a.frames = frames_dev; a.axes = axes_dev;
        a.position = position_dev; a.rotation = rotation_dev; a.jacobian = jacobian_dev;
        a.points = (long long)rows * T; a.D = D;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "motion_pose", [&] { launch_motion_pose(a, s); });
    });
}

int avae_motion_ik(avae_handle* h, const float* path_dev, int32_t rows, int32_t T, int32_t D,
                   const float* frames_dev, const float* axes_dev, const float* seed_dev,
                   const float* orient_dev, int32_t orient_rows, const float* limits_dev,
                   int32_t n_iters, float tol, float rot_tol, float damping, float max_step,
                   float* traj_dev, float* residual_dev, float* rot_residual_dev, int32_t* iterations_dev, int32_t* status_dev,
                   void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_motion_ik";
        check_rows(w, rows, "rows");
        check_range(w, "T", T, 1, kIkMaxT);
        check_range(w, "D", D, 1, kIkMaxD);
        check_range(w, "n_iters", n_iters, 0, kIkMaxIters);
        check_finite(w, "damping", damping, true);
        check_finite(w, "max_step", max_step, true);
        check_finite(w, "tol", tol, false);
        check_finite(w, "rot_tol", rot_tol, false);
        if (orient_dev && orient_rows != 1 && orient_rows != rows)
            throw Err(w + ": orient_rows = " + std::to_string(orient_rows) + " must be 1 or rows = " + std::to_string(rows));
        need(w, path_dev, "path_dev"); need(w, frames_dev, "frames_dev"); need(w, axes_dev, "axes_dev");
        need(w, seed_dev, "seed_dev"); need(w, traj_dev, "traj_dev");
        if (rows == 0) return;
        IkArgs a = zeroed<IkArgs>();
        a.path = path_dev; a.frames = frames_dev; a.axes = axes_dev; a.seed = seed_dev; a.orient = orient_dev; a.limits = limits_dev;
        a.traj = traj_dev; a.residual = residual_dev; a.rot_residual = rot_residual_dev; a.iterations = iterations_dev;
        a.status = status_dev;
        a.tol = tol; a.rot_tol = rot_tol; a.damping = damping; a.max_step = max_step;
        a.rows = rows; a.T = T; a.D = D; a.n_iters = n_iters; a.orient_per_row = orient_dev && orient_rows == rows && rows > 1 ? 1 : 0;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "motion_ik", [&] { launch_motion_ik(a, s); });
    });
}

// ---- joint-space inertia and inverse dynamics (include/avae.h, avae_dynamics.h)
int avae_motion_dynamics(avae_handle* h, const float* traj_dev, const float* vel_dev, const float* acc_dev,
                         int32_t rows, int32_t T, int32_t D, const float* frames_dev, const float* axes_dev,
                         const float* bodies_dev, const float* gravity,
                         float* inertia_dev, float* gravity_dev, float* coriolis_dev, float* torque_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_motion_dynamics";
        check_rows(w, rows, "rows");
        check_range(w, "T", T, 1, kIkMaxT);
        check_range(w, "D", D, 1, kIkMaxD);
        need(w, traj_dev, "traj_dev"); need(w, frames_dev, "frames_dev"); need(w, axes_dev, "axes_dev");
        need(w, bodies_dev, "bodies_dev"); need(w, gravity, "gravity");
        for (int i = 0; i < 3; ++i)
            if (!std::isfinite(gravity[i])) throw Err(w + ": gravity[" + std::to_string(i) + "] must be finite");
        if (!inertia_dev && !gravity_dev && !coriolis_dev && !torque_dev) throw Err(w + ": every output is NULL");
        if (rows == 0) return;
        DynArgs a = zeroed<DynArgs>();
        a.traj = traj_dev; a.vel = vel_dev; a.acc = acc_dev; a.frames = frames_dev; a.axes = axes_dev; a.bodies = bodies_dev;
        a.inertia = inertia_dev; a.gravity = gravity_dev; a.coriolis = coriolis_dev; a.torque = torque_dev;
        a.points = (long long)rows * T; a.D = D;
        for (int i = 0; i < 3; ++i) a.g[i] = -gravity[i];
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "motion_dynamics", [&] { launch_motion_dynamics(a, s); });
    });
}

// ---- sigma-lognormal strokes (include/avae.h, avae_lognormal.h)
static void check_lognormal_shape(const std::string& w, int32_t rows, int32_t C, int32_t T, float dt) {
    check_rows(w, rows, "rows");
    check_range(w, "C", C, 1, kLnMaxC);
    check_range(w, "T", T, 1, kLnMaxT);
    check_finite(w, "dt", dt, true);
}

int avae_lognormal_eval(avae_handle* h, const float* params_dev, const int32_t* count_dev, const float* start_dev,
                        int32_t rows, int32_t C, int32_t T, float dt, float* path_dev, float* velocity_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_lognormal_eval";
        check_lognormal_shape(w, rows, C, T, dt);
        need(w, params_dev, "params_dev"); need(w, start_dev, "start_dev"); need(w, path_dev, "path_dev");
        if (rows == 0) return;
        LnEvalArgs a = zeroed<LnEvalArgs>();
        a.params = params_dev; a.count = count_dev; a.start = start_dev; a.path = path_dev; a.velocity = velocity_dev;
        a.dt = dt; a.rows = rows; a.C = C; a.T = T;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "lognormal_eval", [&] { launch_lognormal_eval(a, s); });
    });
}

int avae_lognormal_sample(avae_handle* h, const float* params_dev, const int32_t* count_dev, const float* start_dev,
                          int32_t rows, int32_t S, int32_t C, int32_t T, float dt, uint64_t seed, int64_t row_offset,
                          float amplitude, float angle, float straightness, int32_t shift_mean,
                          float* strokes_dev, float* perturbed_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_lognormal_sample";
        check_lognormal_shape(w, rows, C, T, dt);
        check_range(w, "S", S, 1, 1 << 20);
        if ((long long)rows * S > 0x7fffffffLL) throw Err(w + ": rows * S is too large for one launch");
        if (row_offset < 0 || row_offset + (int64_t)rows > ((int64_t)1 << 32))
            throw Err(w + ": row_offset = " + std::to_string(row_offset) + " must be >= 0 and row_offset + rows <= 2^32");
        check_finite(w, "amplitude", amplitude, false);
        check_finite(w, "angle", angle, false);
        check_finite(w, "straightness", straightness, false);
        need(w, params_dev, "params_dev"); need(w, start_dev, "start_dev"); need(w, strokes_dev, "strokes_dev");
        if (rows == 0) return;
        LnSampleArgs a = zeroed<LnSampleArgs>();
        a.params = params_dev; a.count = count_dev; a.start = start_dev; a.strokes = strokes_dev; a.perturbed = perturbed_dev;
        a.seed = seed; a.row0 = (unsigned)row_offset; a.dt = dt; a.amplitude = amplitude; a.angle = angle; a.straightness = straightness;
        a.rows = rows; a.S = S; a.C = C; a.T = T; a.shift_mean = shift_mean ? 1 : 0;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "lognormal_sample", [&] { launch_lognormal_sample(a, s); });
    });
}

int avae_lognormal_fit(avae_handle* h, const float* target_dev, const float* init_dev, const int32_t* count_dev,
                       const float* start_dev, int32_t rows, int32_t C, int32_t T, float dt, int32_t n_iters,
                       double wp, double wv, double tol, const uint8_t* free_dev, int32_t free_per_row,
                       const float* lo_dev, const float* hi_dev,
                       float* params_dev, double* loss0_dev, double* loss_dev, int32_t* iterations_dev, int32_t* accepted_dev,
                       int32_t* status_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_lognormal_fit";
        check_lognormal_shape(w, rows, C, T, dt);
        check_range(w, "n_iters", n_iters, 0, kLnMaxIters);
        check_finite(w, "wp", wp, false);
        check_finite(w, "wv", wv, false);
        check_finite(w, "tol", tol, false);
        need(w, target_dev, "target_dev"); need(w, init_dev, "init_dev"); need(w, start_dev, "start_dev");
        need(w, params_dev, "params_dev");
        if (rows == 0) return;
        LnFitArgs a = zeroed<LnFitArgs>();
        a.target = target_dev; a.init = init_dev; a.count = count_dev; a.start = start_dev; a.free_mask = free_dev;
        a.lo = lo_dev; a.hi = hi_dev; a.params = params_dev; a.loss0 = loss0_dev; a.loss = loss_dev;
        a.iterations = iterations_dev; a.accepted = accepted_dev; a.status = status_dev;
        a.wp = wp; a.wv = wv; a.tol = tol; a.dt = dt;
        a.rows = rows; a.C = C; a.T = T; a.n_iters = n_iters; a.free_per_row = free_dev && free_per_row ? 1 : 0;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "lognormal_fit", [&] { launch_lognormal_fit(a, s); });
    });
}

// ---- joint-trajectory synthesis by iLQR (include/avae.h, avae_track.h)
static void check_track_shape(const std::string& w, int32_t rows, int32_t T, int32_t D) {
    check_rows(w, rows, "rows");
    check_range(w, "T", T, 1, kTrackMaxT);
    check_range(w, "D", D, 1, kTrackMaxD);
}

int avae_motion_track_plan(int32_t rows, int32_t T, int32_t D, size_t* workspace_bytes) {
    try {
        const std::string w = "avae_motion_track_plan";
        check_track_shape(w, rows, T, D);
        need(w, workspace_bytes, "workspace_bytes");
        *workspace_bytes = (size_t)rows * track_row_bytes(T, D);
        return 0;
    } catch (const std::exception& e) { g_create_error = e.what(); return 2; }
}

int avae_motion_track(avae_handle* h, const float* path_dev, const float* init_dev, int32_t rows, int32_t T, int32_t D,
                      const float* frames_dev, const float* axes_dev, float dt, const float* track_w, float R,
                      const float* effort_dev, const float* limits_dev, float limit_weight,
                      int32_t n_iters, double lam0, double factor, double lam_min, double lam_max, double tol,
                      void* workspace_dev, size_t workspace_bytes,
                      float* traj_dev, float* controls_dev, double* cost0_dev, double* cost_dev, float* track_rmse_dev,
                      int32_t* iterations_dev, int32_t* accepted_dev, int32_t* status_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_motion_track";
        check_track_shape(w, rows, T, D);
        check_range(w, "n_iters", n_iters, 0, kTrackMaxIters);
        check_finite(w, "dt", dt, true);
        need(w, track_w, "track_w");
        for (int i = 0; i < 3; ++i) check_finite(w, "track_w", track_w[i], false);
        check_finite(w, "R", R, false);
        check_finite(w, "limit_weight", limit_weight, false);
        check_finite(w, "lam0", lam0, true);
        check_finite(w, "factor - 1", factor - 1.0, true);
        check_finite(w, "lam_min", lam_min, true);
        if (!std::isfinite(lam_max) || lam_max < lam0) throw Err(w + ": lam_max must be finite and >= lam0");
        check_finite(w, "tol", tol, false);
        need(w, path_dev, "path_dev"); need(w, init_dev, "init_dev"); need(w, frames_dev, "frames_dev"); need(w, axes_dev, "axes_dev");
        need(w, traj_dev, "traj_dev");
        if (rows == 0) return;
        const size_t row_bytes = track_row_bytes(T, D);
        need(w, workspace_dev, "workspace_dev");
        if (workspace_bytes < (size_t)rows * row_bytes)
            throw Err(w + ": workspace_bytes = " + std::to_string(workspace_bytes) + " is below the " +
                      std::to_string((size_t)rows * row_bytes) + " bytes avae_motion_track_plan gives");
        if (reinterpret_cast<uintptr_t>(workspace_dev) % 8 != 0) throw Err(w + ": workspace_dev must be aligned to 8 bytes");
        TrackArgs a = zeroed<TrackArgs>();
        a.path = path_dev; a.init = init_dev; a.frames = frames_dev; a.axes = axes_dev; a.effort = effort_dev;
        a.limits = limit_weight > 0.0f ? limits_dev : nullptr;                                       // (limits nobody reads)
        a.workspace = static_cast<unsigned char*>(workspace_dev);
        a.traj = traj_dev; a.controls = controls_dev; a.cost0 = cost0_dev; a.cost = cost_dev; a.rmse = track_rmse_dev;
        a.iterations = iterations_dev; a.accepted = accepted_dev; a.status = status_dev;
        a.lam0 = lam0; a.factor = factor; a.lam_min = lam_min; a.lam_max = lam_max; a.tol = tol;
        a.row_bytes = row_bytes;
        a.dt = dt; a.w[0] = track_w[0]; a.w[1] = track_w[1]; a.w[2] = track_w[2]; a.R = R; a.limit_weight = limit_weight;
        a.rows = rows; a.T = T; a.D = D; a.n_iters = n_iters;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "motion_track", [&] { launch_motion_track(a, s); });
    });
}

// ---- black-box search (include/avae.h, avae_search.h)
static void check_search_shape(const std::string& w, int32_t P, int32_t R, int32_t n) {
    check_rows(w, P, "P");
    check_range(w, "R", R, 1, kSearchMaxR);
    check_range(w, "n", n, 1, kSearchMaxN);
}

int avae_search_sample(avae_handle* h, const float* mean_dev, const float* var_dev, int32_t P, int32_t R, int32_t n,
                       uint64_t seed, int32_t iteration, int64_t problem_offset,
                       const float* proj_A_dev, const float* proj_b_dev, int32_t G, int32_t g, float* x_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_search_sample";
        check_search_shape(w, P, R, n);
        if (iteration < 0) throw Err(w + ": iteration = " + std::to_string(iteration) + " must be >= 0");
        if (problem_offset < 0 || problem_offset + (int64_t)P > ((int64_t)1 << 32))
            throw Err(w + ": problem_offset = " + std::to_string(problem_offset) + " must be >= 0 and problem_offset + P <= 2^32");
        if ((proj_A_dev != nullptr) != (proj_b_dev != nullptr)) throw Err(w + ": proj_A_dev and proj_b_dev go together; one of them is NULL");
        if (proj_A_dev) {
            check_range(w, "g", g, 1, kSearchMaxG);
            if (G < 1 || (long long)G * g != n)
                throw Err(w + ": G * g = " + std::to_string(G) + " * " + std::to_string(g) + " must be n = " + std::to_string(n));
        }
        need(w, mean_dev, "mean_dev"); need(w, var_dev, "var_dev"); need(w, x_dev, "x_dev");
        if (P == 0) return;
        static_assert(kSearchTileFloats >= 4 * ((kSearchMaxN + 3) / 4), "a sample tile holds at least one row");
        SearchSampleArgs a = zeroed<SearchSampleArgs>();
        a.mean = mean_dev; a.var = var_dev; a.proj_A = proj_A_dev; a.proj_b = proj_b_dev; a.x = x_dev;
        a.rows = (long long)P * R; a.seed = seed; a.problem0 = (unsigned)problem_offset; a.iteration = (unsigned)iteration;
        a.R = R; a.n = n; a.G = proj_A_dev ? G : 0; a.g = proj_A_dev ? g : 0;
        if ((a.rows + search_tile_rows(n) - 1) / search_tile_rows(n) > 0x7fffffffLL) throw Err(w + ": P * R is too large for one launch");
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "search_sample", [&] { launch_search_sample(a, s); });
    });
}

int avae_search_update(avae_handle* h, const float* x_dev, const float* cost_dev, int32_t P, int32_t R, int32_t n,
                       const avae_search_options* opt,
                       float* mean_dev, float* var_dev, int32_t* n_applied_dev, int32_t* frozen_dev,
                       float* best_cost_dev, float* best_x_dev,
                       float* avg_cost_dev, float* min_cost_dev, float* moved_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_search_update";
        check_search_shape(w, P, R, n);
        need(w, opt, "opt");
        if (opt->weighting != AVAE_SEARCH_PIBB && opt->weighting != AVAE_SEARCH_CEM && opt->weighting != AVAE_SEARCH_CMAES)
            throw Err(w + ": weighting = " + std::to_string(opt->weighting) + " is none of AVAE_SEARCH_PIBB, _CEM, _CMAES");
        if (opt->cov_update != AVAE_SEARCH_PIBB && opt->cov_update != AVAE_SEARCH_CEM)
            throw Err(w + ": cov_update = " + std::to_string(opt->cov_update) + " is neither AVAE_SEARCH_PIBB nor AVAE_SEARCH_CEM");
        check_finite(w, "eliteness", opt->eliteness, false);
        if (opt->weighting != AVAE_SEARCH_PIBB && (opt->eliteness < 1.0 || opt->eliteness > 1e9 || opt->eliteness != std::floor(opt->eliteness)))
            throw Err(w + ": eliteness must be a whole number >= 1 for CEM / CMA-ES weighting (the number of rollouts kept)");
        if (!(opt->learning_rate >= 0.0 && opt->learning_rate <= 1.0)) throw Err(w + ": learning_rate must be in [0, 1]");
        if (!std::isfinite(opt->rel_lower) || !std::isfinite(opt->abs_lower) || !std::isfinite(opt->abs_upper))
            throw Err(w + ": rel_lower, abs_lower and abs_upper must be finite (negative: off)");
        if (opt->rel_lower > 1.0) throw Err(w + ": rel_lower must be <= 1");
        check_finite(w, "tol", opt->tol, false);
        need(w, x_dev, "x_dev"); need(w, cost_dev, "cost_dev"); need(w, mean_dev, "mean_dev"); need(w, var_dev, "var_dev");
        need(w, n_applied_dev, "n_applied_dev"); need(w, frozen_dev, "frozen_dev");
        need(w, best_cost_dev, "best_cost_dev"); need(w, best_x_dev, "best_x_dev");
        if (P == 0) return;
        SearchUpdateArgs a = zeroed<SearchUpdateArgs>();
        a.x = x_dev; a.cost = cost_dev; a.mean = mean_dev; a.var = var_dev; a.n_applied = n_applied_dev; a.frozen = frozen_dev;
        a.best_cost = best_cost_dev; a.best_x = best_x_dev; a.avg_cost = avg_cost_dev; a.min_cost = min_cost_dev; a.moved = moved_dev;
        a.R = R; a.n = n; a.weighting = opt->weighting; a.cov_update = opt->cov_update;
        a.mu = opt->weighting != AVAE_SEARCH_PIBB ? (int)opt->eliteness : 0;
        a.h = opt->eliteness; a.lr = opt->learning_rate; a.rel_lower = opt->rel_lower; a.abs_lower = opt->abs_lower;
        a.abs_upper = opt->abs_upper; a.tol = opt->tol;
        hipStream_t s = on_stream(h, stream);
        timed_launch(h, s, "search_update", [&] { launch_search_update(a, P, s); });
    });
}

// ---- aggregate-posterior log-density (include/avae.h, avae_aggpost.h)
static void check_agg_shape(const std::string& w, int32_t rows, int32_t gallery_rows) {
    check_rows(w, rows, "rows");
    check_rows(w, gallery_rows, "gallery_rows");
}

int avae_agg_logpdf_plan(const avae_config* cfg, int32_t rows, int32_t gallery_rows, int32_t* query_tile, int32_t* chunk_rows,
                         int32_t* slice_rows, int32_t* n_slices, size_t* scratch_bytes) {
    return plan_query(cfg, [&] {
        check_agg_shape("avae_agg_logpdf_plan", rows, gallery_rows);
        const AggPlan p = agg_plan(rows, gallery_rows);
        put(query_tile, p.query_tile); put(chunk_rows, p.chunk_rows); put(slice_rows, p.slice_rows); put(n_slices, p.n_slices);
        put(scratch_bytes, agg_scratch_bytes(p, cfg->n_z));
    });
}

int avae_agg_logpdf(avae_handle* h, const float* z_dev, int32_t rows, const float* g_mu_dev, const float* g_logvar_dev,
                    int32_t gallery_rows, const int32_t* exclude_dev, float* joint_dev, float* marginal_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_agg_logpdf";
        check_agg_shape(w, rows, gallery_rows);
        if (rows > 0) need(w, z_dev, "z_dev");
        if (gallery_rows > 0) { need(w, g_mu_dev, "g_mu_dev"); need(w, g_logvar_dev, "g_logvar_dev"); }
        if (!joint_dev && !marginal_dev) throw Err(w + ": joint_dev and marginal_dev are both NULL");
        if (rows == 0) return;
        static_assert(kAggMaxNz >= 64, "check_config bounds n_z by 64");
        const int nz = h->nz;
        const AggPlan p = agg_plan(rows, gallery_rows);
        hipStream_t s = on_stream(h, stream);
        AggArgs a = zeroed<AggArgs>();
        a.g_mu = g_mu_dev; a.g_lv = g_logvar_dev; a.gallery_rows = gallery_rows; a.nz = nz;
        a.n_slices = p.n_slices; a.slice_rows = p.slice_rows;
        if (p.n_slices > 0) a.part = scratch_of<float2>(h->agg_buf, w, agg_scratch_bytes(p, nz), kAggScratchBytes, agg_lds_bytes(nz));
        for (int r0 = 0; r0 < rows; r0 += p.chunk_rows) {
            a.rows = std::min(p.chunk_rows, rows - r0);
            a.z = z_dev + (size_t)r0 * nz;
            a.exclude = exclude_dev ? exclude_dev + r0 : nullptr;
            a.joint = joint_dev ? joint_dev + r0 : nullptr;
            a.marginal = marginal_dev ? marginal_dev + (size_t)r0 * nz : nullptr;
            if (p.n_slices > 0) timed_launch(h, s, "agg_logpdf", [&] { launch_agg_logpdf(a, s); });
            timed_launch(h, s, "agg_logpdf_merge", [&] { launch_agg_logpdf_merge(a, s); });
        }
    });
}

// ---- mixture prior fitted to the posteriors (include/avae.h, avae_gmm.h)
static void check_gmm_shape(const std::string& w, int32_t rows, int32_t K) {
    check_rows(w, rows, "rows");
    if (K < 1 || K > kGmmMaxK)
        throw Err(w + ": n_components = " + std::to_string(K) + " must be in [1, " + std::to_string(kGmmMaxK) + "]");
}

int avae_gmm_plan(const avae_config* cfg, int32_t rows, int32_t n_components, int32_t* slice_rows, int32_t* n_slices,
                  size_t* scratch_bytes) {
    return plan_query(cfg, [&] {
        check_gmm_shape("avae_gmm_plan", rows, n_components);
        const GmmPlan p = gmm_plan(rows);
        put(slice_rows, p.slice_rows); put(n_slices, p.n_slices);
        put(scratch_bytes, gmm_scratch_bytes(p.n_slices, n_components, cfg->n_z));
    });
}

int avae_gmm_fit(avae_handle* h, const float* mu_dev, const float* logvar_dev, int32_t rows, int32_t n_components, int32_t n_iters,
                 float var_floor, float* weights_dev, float* means_dev, float* logvars_dev, double* bound_dev, int32_t* n_used_dev,
                 void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_gmm_fit";
        check_gmm_shape(w, rows, n_components);
        if (n_iters < 0) throw Err(w + ": n_iters must be >= 0");
        if (!(var_floor > 0.0f) || !std::isfinite(var_floor)) throw Err(w + ": var_floor must be positive and finite");
        if (rows > 0) need(w, mu_dev, "mu_dev");
        need(w, weights_dev, "weights_dev"); need(w, means_dev, "means_dev"); need(w, logvars_dev, "logvars_dev");
        need(w, bound_dev, "bound_dev"); need(w, n_used_dev, "n_used_dev");
        static_assert(kGmmMaxNz >= 64, "check_config bounds n_z by 64");
        const int nz = h->nz, K = n_components;
        const GmmPlan p = gmm_plan(rows);
        hipStream_t s = on_stream(h, stream);
        GmmArgs a = zeroed<GmmArgs>();
        a.mu = mu_dev; a.lv = logvar_dev; a.rows = rows; a.nz = nz; a.K = K;
        a.n_slices = p.n_slices; a.slice_rows = p.slice_rows; a.var_floor = var_floor; a.n_used = n_used_dev;
        a.part = scratch_of<double>(h->gmm_buf, w, gmm_scratch_bytes(p.n_slices, K, nz), kGmmScratchBytes, gmm_lds_bytes(K, nz));
        // iteration t reads the set iteration t - 1 wrote: the caller's arrays first, the scratch's two sets in turn between, and the
        // last one writes the caller's arrays again (every element is read and written by the same thread where the two coincide)
        const size_t pf = gmm_param_floats(K, nz);
        float* sets[2];
        sets[0] = reinterpret_cast<float*>(a.part + (size_t)kGmmMaxSlices * gmm_part_stride(kGmmMaxK, kGmmMaxNz));
        sets[1] = sets[0] + pf;
        auto point = [&](float* base, float*& pw, float*& pmean, float*& ps) { pw = base; pmean = base + K; ps = base + K + (size_t)K * nz; };
        const float *wi = weights_dev, *mi = means_dev, *si = logvars_dev;
        for (int t = 0; t <= n_iters; ++t) {
            const bool last = t == n_iters;
            a.w_in = wi; a.m_in = mi; a.s_in = si;
            a.want_stats = last ? 2 : 1; a.final_pass = last ? 1 : 0;
            a.bound = bound_dev + t;
            if (last) { a.w_out = nullptr; a.m_out = nullptr; a.s_out = nullptr; }
            else if (t == n_iters - 1) { a.w_out = weights_dev; a.m_out = means_dev; a.s_out = logvars_dev; }
            else point(sets[t & 1], a.w_out, a.m_out, a.s_out);
            if (p.n_slices > 0) timed_launch(h, s, "gmm_estep", [&] { launch_gmm_estep(a, s); });
            timed_launch(h, s, "gmm_mstep", [&] { launch_gmm_mstep(a, s); });
            wi = a.w_out; mi = a.m_out; si = a.s_out;
        }
    });
}

int avae_gmm_score(avae_handle* h, const float* mu_dev, const float* logvar_dev, int32_t rows, int32_t n_components,
                   const float* weights_dev, const float* means_dev, const float* logvars_dev, float* ll_dev, int32_t* component_dev,
                   float* resp_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_gmm_score";
        check_gmm_shape(w, rows, n_components);
        if (rows > 0) need(w, mu_dev, "mu_dev");
        need(w, weights_dev, "weights_dev"); need(w, means_dev, "means_dev"); need(w, logvars_dev, "logvars_dev");
        if (!ll_dev && !component_dev && !resp_dev) throw Err(w + ": ll_dev, component_dev and resp_dev are all NULL");
        if (rows == 0) return;
        const int nz = h->nz;
        const GmmPlan p = gmm_plan(rows);
        if (gmm_lds_bytes(n_components, nz) > kMaxDynLds) throw Err("internal error: " + w + " plans more LDS than its bound");
        hipStream_t s = on_stream(h, stream);
        GmmArgs a = zeroed<GmmArgs>();
        a.mu = mu_dev; a.lv = logvar_dev; a.rows = rows; a.nz = nz; a.K = n_components;
        a.n_slices = p.n_slices; a.slice_rows = p.slice_rows;
        a.w_in = weights_dev; a.m_in = means_dev; a.s_in = logvars_dev;
        a.ll = ll_dev; a.component = component_dev; a.resp = resp_dev;
        timed_launch(h, s, "gmm_score", [&] { launch_gmm_estep(a, s); });
    });
}

// ---- 2-D t-SNE map of the posteriors (include/avae.h, avae_embed.h)
static bool check_embed_shape(const std::string& w, int32_t rows, int32_t metric) {
    check_rows(w, rows, "rows");
    if (rows > kEmbedMaxRows)
        throw Err(w + ": rows = " + std::to_string(rows) + " is more than " + std::to_string(kEmbedMaxRows) + " (the work is quadratic in rows)");
    return check_metric(w, metric);
}

int avae_embed_plan(const avae_config* cfg, int32_t rows, int32_t* row_tile, int32_t* n_splits, int32_t* tiles_per_split,
                    size_t* scratch_bytes) {
    return plan_query(cfg, [&] {
        check_embed_shape("avae_embed_plan", rows, AVAE_METRIC_L2);
        const EmbedPlan p = embed_plan(rows);
        put(row_tile, p.row_tile); put(n_splits, p.n_splits); put(tiles_per_split, p.tiles_per_split);
        put(scratch_bytes, p.scratch_bytes);
    });
}

// the fields every launch of the family reads, and the scratch
static EmbedArgs embed_args(avae_handle* h, const std::string& w, const float* mu_dev, const float* logvar_dev, int32_t rows, bool kl) {
    static_assert(kEmbedMaxNz >= 64, "check_config bounds n_z by 64");
    const EmbedPlan p = embed_plan(rows);
    const int metric = kl ? AVAE_METRIC_SYMKL : AVAE_METRIC_L2;
    static_assert(kEmbedOffPart + (kEmbedParts + 1) * kEmbedMaxSlots * sizeof(double) == kEmbedScratchBytes, "the bytes bound the slots");
    unsigned char* base = scratch_of<unsigned char>(h->embed_buf, w, p.scratch_bytes, kEmbedScratchBytes, embed_lds_bytes(h->nz, metric));
    EmbedArgs a = zeroed<EmbedArgs>();
    a.mu = mu_dev; a.lv = kl ? logvar_dev : nullptr;           // the L2 metric never reads the log-variances
    a.rows = rows; a.nz = h->nz; a.metric = metric;
    a.n_splits = p.n_splits; a.tiles_per_split = p.tiles_per_split;
    a.used = base;
    a.count = reinterpret_cast<int32_t*>(base + kEmbedOffCount);
    a.mean = reinterpret_cast<double*>(base + kEmbedOffMean);
    a.part = reinterpret_cast<double*>(base + kEmbedOffPart);
    a.part_stride = (size_t)rows * p.n_splits;
    a.plogp = a.part + (size_t)kEmbedParts * a.part_stride;
    return a;
}

int avae_embed_calibrate(avae_handle* h, const float* mu_dev, const float* logvar_dev, int32_t rows, int32_t metric, double perplexity,
                         double tol, int32_t max_tries, float* beta_dev, float* shift_dev, float* norm_dev, int32_t* tries_dev,
                         int32_t* n_used_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_embed_calibrate";
        const bool kl = check_embed_shape(w, rows, metric);
        if (rows == 0) return;
        if (!(perplexity >= 1.0 && perplexity <= (double)(rows - 1)))
            throw Err(w + ": perplexity must be in [1, rows - 1] = [1, " + std::to_string(rows - 1) + "]");
        if (!(tol > 0.0)) throw Err(w + ": tol must be > 0");
        if (max_tries < 1) throw Err(w + ": max_tries must be >= 1");
        need(w, mu_dev, "mu_dev");
        if (kl) need(w, logvar_dev, "logvar_dev", kNeedsLogvar);
        need(w, beta_dev, "beta_dev"); need(w, shift_dev, "shift_dev"); need(w, norm_dev, "norm_dev");
        need(w, tries_dev, "tries_dev"); need(w, n_used_dev, "n_used_dev");
        EmbedArgs a = embed_args(h, w, mu_dev, logvar_dev, rows, kl);
        hipStream_t s = on_stream(h, stream);
        a.beta = beta_dev; a.shift = shift_dev; a.norm = norm_dev; a.tries = tries_dev; a.n_used = n_used_dev;
        a.log_perp = std::log(perplexity); a.tol = tol; a.max_tries = max_tries;
        timed_launch(h, s, "embed_scan", [&] { launch_embed_scan(a, s); });
        timed_launch(h, s, "embed_calibrate", [&] { launch_embed_calibrate(a, s); });
    });
}

int avae_embed_iterate(avae_handle* h, const float* mu_dev, const float* logvar_dev, int32_t rows, int32_t metric, const float* beta_dev,
                       const float* shift_dev, const float* norm_dev, float* y_dev, float* vel_dev, float* gain_dev, int32_t it0,
                       int32_t n_iters, float learning_rate, float early_exaggeration, int32_t exaggeration_iters, float momentum0,
                       float momentum1, int32_t center, double* kl_dev, float* grad_dev, void* stream) {
    return guarded(h, [&] {
        const std::string w = "avae_embed_iterate";
        const bool kl = check_embed_shape(w, rows, metric);
        if (rows == 0) return;
        if (n_iters < 0) throw Err(w + ": n_iters must be >= 0");
        if (it0 < 0) throw Err(w + ": it0 must be >= 0");
        if (!(learning_rate > 0.0f) || !std::isfinite(learning_rate)) throw Err(w + ": learning_rate must be positive and finite");
        need(w, mu_dev, "mu_dev");
        if (kl) need(w, logvar_dev, "logvar_dev", kNeedsLogvar);
        need(w, beta_dev, "beta_dev"); need(w, shift_dev, "shift_dev"); need(w, norm_dev, "norm_dev");
        need(w, y_dev, "y_dev"); need(w, vel_dev, "vel_dev"); need(w, gain_dev, "gain_dev"); need(w, kl_dev, "kl_dev");
        EmbedArgs a = embed_args(h, w, mu_dev, logvar_dev, rows, kl);
        hipStream_t s = on_stream(h, stream);
        a.beta = const_cast<float*>(beta_dev); a.shift = const_cast<float*>(shift_dev); a.norm = const_cast<float*>(norm_dev);
        a.y = y_dev; a.vel = vel_dev; a.gain = gain_dev; a.lr = learning_rate;
        timed_launch(h, s, "embed_scan", [&] { launch_embed_scan(a, s); });
        for (int i = 0; i <= n_iters; ++i) {
            const long long t = (long long)it0 + i;
            const bool last = i == n_iters;
            a.first_pass = i == 0 ? 1 : 0;
            a.evaluate = last ? 1 : 0;
            a.center = last && center != 0 && n_iters > 0 ? 1 : 0;
            a.alpha = t < exaggeration_iters ? early_exaggeration : 1.0f;
            a.mom = t < exaggeration_iters ? momentum0 : momentum1;
            a.kl = kl_dev + i;
            a.grad = i == 0 ? grad_dev : nullptr;
            timed_launch(h, s, "embed_forces", [&] { launch_embed_forces(a, s); });
            timed_launch(h, s, "embed_update", [&] { launch_embed_update(a, s); });
            if (a.center) timed_launch(h, s, "embed_center", [&] { launch_embed_center(a, s); });
        }
    });
}

// ---- checkpoint: "AVAECKPT" | u32 version | u32 n_mod | u32 n_z | per modality {n_input, L, hs[L], conv, gener1, gener2} | u64 P | i64 step | theta | m | v
// version 2: that; version 3 (written while parameter averaging is on): that, then f32 decay | u32 warmup | the average [P]
int avae_save(avae_handle* h, const char* path) {
    return guarded(h, [&] {
        std::vector<float> I, th(h->P_flat), mm(h->P_flat), vv(h->P_flat), av;
        if (h->ema_on) { av.resize(h->P_flat); ema_to_host(h, I); convert_params<false>(h, av.data(), I.data()); }
        master_to_host(h, h->off_theta, I); convert_params<false>(h, th.data(), I.data());
        master_to_host(h, h->off_m, I); convert_params<false>(h, mm.data(), I.data());
        master_to_host(h, h->off_v, I); convert_params<false>(h, vv.data(), I.data());
        long long step = 0;
        HIP_OK(hipMemcpy(&step, &h->state()->step, sizeof(step), hipMemcpyDeviceToHost));
        FILE* f = std::fopen(path, "wb");
        if (!f) throw Err(std::string("cannot open for writing: ") + path);
        auto w32 = [&](uint32_t v) { std::fwrite(&v, 4, 1, f); };
        std::fwrite("AVAECKPT", 1, 8, f);
        w32(h->ema_on ? 3 : 2); w32((uint32_t)h->M); w32((uint32_t)h->nz);
        for (int m = 0; m < h->M; ++m) {
            const Mod& md = h->mods[m];
            w32((uint32_t)md.n_in); w32((uint32_t)md.hs.size()); for (int x : md.hs) w32((uint32_t)x);
            w32(md.conv ? 1u : 0u); w32((uint32_t)h->cfg.mod[m].conv_gener[0]); w32((uint32_t)h->cfg.mod[m].conv_gener[1]);
        }
        uint64_t P = h->P_flat; std::fwrite(&P, 8, 1, f);
        int64_t st = step; std::fwrite(&st, 8, 1, f);
        bool ok = std::fwrite(th.data(), 4, P, f) == P && std::fwrite(mm.data(), 4, P, f) == P && std::fwrite(vv.data(), 4, P, f) == P;
        if (h->ema_on) {
            const float decay = h->ema_decay;
            ok = std::fwrite(&decay, 4, 1, f) == 1 && ok;
            w32((uint32_t)h->ema_warmup);
            ok = std::fwrite(av.data(), 4, P, f) == P && ok;
        }
        ok = (std::fclose(f) == 0) && ok;
        if (!ok) throw Err(std::string("short write: ") + path);
    });
}

int avae_load(avae_handle* h, const char* path) {
    return guarded(h, [&] {
        FILE* f = std::fopen(path, "rb");
        if (!f) throw Err(std::string("cannot open for reading: ") + path);
        std::vector<float> th, mm, vv, av;
        int64_t st = 0;
        uint32_t version = 0, warmup = 0;
        float decay = 0.0f;
        try {
            char magic[8];
            auto r32 = [&]() { uint32_t v = 0; if (std::fread(&v, 4, 1, f) != 1) throw Err("truncated checkpoint"); return v; };
            if (std::fread(magic, 1, 8, f) != 8 || std::memcmp(magic, "AVAECKPT", 8) != 0) throw Err("not an AVAE checkpoint");
            version = r32();
            if (version != 2 && version != 3) throw Err("unsupported checkpoint version");
            if ((int)r32() != h->M || (int)r32() != h->nz) throw Err("checkpoint architecture mismatch (modalities / n_z)");
            for (int m = 0; m < h->M; ++m) {
                const Mod& md = h->mods[m];
                if ((int)r32() != md.n_in || r32() != (uint32_t)md.hs.size()) throw Err("checkpoint architecture mismatch (n_input / depth)");
                for (int x : md.hs) if ((int)r32() != x) throw Err("checkpoint architecture mismatch (hidden width)");
                const bool conv = r32() != 0;
                const int g1 = (int)r32(), g2 = (int)r32();
                if (conv != md.conv || (conv && (g1 != h->cfg.mod[m].conv_gener[0] || g2 != h->cfg.mod[m].conv_gener[1])))
                    throw Err("checkpoint architecture mismatch (conv branch)");
            }
            uint64_t P = 0;
            if (std::fread(&P, 8, 1, f) != 1 || P != h->P_flat) throw Err("checkpoint parameter count mismatch");
            if (std::fread(&st, 8, 1, f) != 1) throw Err("truncated checkpoint");
            th.resize(P); mm.resize(P); vv.resize(P);
            if (std::fread(th.data(), 4, P, f) != P || std::fread(mm.data(), 4, P, f) != P || std::fread(vv.data(), 4, P, f) != P)
                throw Err("truncated checkpoint");
            if (version == 3) {
                if (std::fread(&decay, 4, 1, f) != 1) throw Err("truncated checkpoint");
                warmup = r32();
                if (!(decay > 0.0f && decay < 1.0f) || warmup > 1) throw Err("checkpoint holds invalid averaging settings");
                av.resize(P);
                if (std::fread(av.data(), 4, P, f) != P) throw Err("truncated checkpoint");
            }
        } catch (...) { std::fclose(f); throw; }
        std::fclose(f);
        std::vector<float> I(h->P_int, 0.0f);
        convert_params<true>(h, th.data(), I.data()); host_to_master(h, h->off_theta, I);
        std::fill(I.begin(), I.end(), 0.0f); convert_params<true>(h, mm.data(), I.data()); host_to_master(h, h->off_m, I);
        std::fill(I.begin(), I.end(), 0.0f); convert_params<true>(h, vv.data(), I.data()); host_to_master(h, h->off_v, I);
        long long step = st;
        HIP_OK(hipMemcpy(&h->state()->step, &step, sizeof(step), hipMemcpyHostToDevice));
        run_adam(h, 1, nullptr);          // (from theta: avae_use_averaged is off after a load)
        HIP_OK(hipDeviceSynchronize());
        h->averaged = false;
        if (version == 3) {               // the file's settings and average
            set_ema(h, decay, (int32_t)warmup);
            std::fill(I.begin(), I.end(), 0.0f); convert_params<true>(h, av.data(), I.data()); host_to_ema(h, I);
        } else if (h->ema_on) {
            ema_from_theta(h);            // a file without an average: it starts again at the loaded parameters
        }
    });
}

int avae_synchronize(avae_handle* h) {
    return guarded(h, [&] { HIP_OK(hipDeviceSynchronize()); comm_check_error(h); });
}

int avae_timing_enable(avae_handle* h, int32_t on) {
    return guarded(h, [&] {
        HIP_OK(hipDeviceSynchronize());
        for (TimingRec& r : h->trecs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
        h->trecs.clear();
        h->timing = on != 0;
    });
}

// one line per launch name: "<name> <calls> <avg_ms> <min_ms>\n"
int avae_timing_report(avae_handle* h, char* buf, size_t buf_bytes) {
    return guarded(h, [&] {
        HIP_OK(hipDeviceSynchronize());
        // Each interval is the dispatch's own begin -> end (hipExtLaunchKernel events), the times rocprofv3
        // --kernel-trace reports.  While timing is on every step also times a null kernel (one 4-byte store),
        // reported as "_null_kernel": the floor of what one launch can measure.  Nothing is subtracted.
        const double cal_ms = 0.0;
        std::vector<double> sum(h->tnames.size(), 0.0), mn(h->tnames.size(), 1e30);
        std::vector<long> cnt(h->tnames.size(), 0);
        for (TimingRec& r : h->trecs) {
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, r.a, r.b));
            sum[r.launch_name] += ms; cnt[r.launch_name] += 1; mn[r.launch_name] = std::min(mn[r.launch_name], (double)ms);
        }
        std::string out;
        for (size_t i = 0; i < h->tnames.size(); ++i) {
            if (!cnt[i]) continue;
            char line[256];
            std::snprintf(line, sizeof(line), "%s %ld %.6f %.6f\n", h->tnames[i].c_str(), cnt[i], std::max(0.0, sum[i] / cnt[i] - cal_ms), std::max(0.0, mn[i] - cal_ms));
            out += line;
        }
        if (!buf || buf_bytes == 0) throw Err("null buffer");
        std::snprintf(buf, buf_bytes, "%s", out.c_str());
    });
}

int avae_comm_allreduce(avae_handle* h, int32_t bucket, void* stream) {
    return guarded(h, [&] {
        if (!h->comm_on) throw Err("avae_comm_allreduce: the replica has no library-owned collective (use_comm)");
        if (bucket < 0 || bucket >= h->n_buckets) throw Err("data-parallel bucket out of range");
        dp_allreduce(h, bucket, on_stream(h, stream));
    });
}

int avae_debug_fetch(avae_handle* h, const char* name, float* host_dst, size_t max_floats, size_t* n_floats) {
    return guarded(h, [&] {
        std::string n(name ? name : "");
        const void* src = nullptr;
        size_t cnt = 0;
        if (n == "eps") {     // internal rows are padded to a multiple of 4 floats: hand back dense [B][n_z]
            cnt = (size_t)h->B * h->nz;
            if (cnt > max_floats) throw Err("debug_fetch: destination too small");
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy2D(host_dst, (size_t)h->nz * 4, h->at<void>(h->off_eps), (size_t)h->ld_eps * 4, (size_t)h->nz * 4, h->B, hipMemcpyDeviceToHost));
            if (n_floats) *n_floats = cnt;
            return;
        }
#ifdef AVAE_STAMPS
        else if (n == "stamps") { src = h->at<void>(h->off_stamps); cnt = (size_t)kStampLaunches * kStampBlocks * kStampWords * 2; }
#endif
        else if ((n[0] == 'E' || n[0] == 'D') && n.size() >= 4 && n.find('_') != std::string::npos) {
            // "E<m>_<k>" / "D<m>_<k>": the stored output of encoder / decoder hidden layer k of modality m, dense [B][width] as fp32
            // (tests: the relu decisions of the last forward pass)
            const int m = std::atoi(n.c_str() + 1), k = std::atoi(n.c_str() + n.find('_') + 1);
            if (m < 0 || m >= h->M || h->mods[m].conv || k < 0 || k >= h->mods[m].L) throw Err("debug_fetch: no such hidden layer");
            const Act& a = n[0] == 'E' ? h->mods[m].E[k] : h->mods[m].D[k];
            cnt = (size_t)h->B * a.width;
            if (cnt > max_floats) throw Err("debug_fetch: destination too small");
            HIP_OK(hipDeviceSynchronize());
            std::vector<unsigned char> raw((size_t)h->B * a.ld * h->es);
            HIP_OK(hipMemcpy(raw.data(), h->at<void>(a.rm), raw.size(), hipMemcpyDeviceToHost));
            for (int r = 0; r < h->B; ++r)
                for (int c = 0; c < a.width; ++c) {
                    float v;
                    if (h->es == 2) { const uint32_t u = (uint32_t)reinterpret_cast<const uint16_t*>(raw.data())[(size_t)r * a.ld + c] << 16; std::memcpy(&v, &u, 4); }
                    else v = reinterpret_cast<const float*>(raw.data())[(size_t)r * a.ld + c];
                    host_dst[(size_t)r * a.width + c] = v;
                }
            if (n_floats) *n_floats = cnt;
            return;
        }
        else if ((n[0] == 'X' || n[0] == 'T') && n.size() >= 2 && std::isdigit((unsigned char)n[1])) {
            // "X<m>" / "T<m>": staging set 0's encoder input (compute dtype) / exact loss target of modality m, dense [B][n_input] as fp32
            const int m = std::atoi(n.c_str() + 1);
            if (m < 0 || m >= h->M) throw Err("debug_fetch: modality out of range");
            const Mod& md = h->mods[m];
            const bool enc = n[0] == 'X';
            const int ld = enc ? md.X0.ld : md.ld32, esz = enc ? h->es : 4;
            cnt = (size_t)h->B * md.n_in;
            if (cnt > max_floats) throw Err("debug_fetch: destination too small");
            HIP_OK(hipDeviceSynchronize());
            std::vector<unsigned char> raw((size_t)h->B * ld * esz);
            HIP_OK(hipMemcpy(raw.data(), enc ? h->at<void>(md.X0.rm) : h->at<void>(md.X32), raw.size(), hipMemcpyDeviceToHost));
            for (int r = 0; r < h->B; ++r)
                for (int c = 0; c < md.n_in; ++c) {
                    float v;
                    if (esz == 2) { const uint32_t u = (uint32_t)reinterpret_cast<const uint16_t*>(raw.data())[(size_t)r * ld + c] << 16; std::memcpy(&v, &u, 4); }
                    else v = reinterpret_cast<const float*>(raw.data())[(size_t)r * ld + c];
                    host_dst[(size_t)r * md.n_in + c] = v;
                }
            if (n_floats) *n_floats = cnt;
            return;
        }
        else if (n == "shadow_err") {
            // tests: the compute-dtype shadows the optimiser rewrites must BE the parameters (rounded once): W[r][c] and W^T[c][r]
            // against theta[r][c] for every dense layer and conv stage -> {max |W - theta|, max |W^T - theta|, layers checked, worst layer}.
            // A stale or misplaced shadow entry only shows in the NEXT step's arithmetic; this sees it at once, on any configuration.
            if (max_floats < 4) throw Err("debug_fetch: destination too small");
            HIP_OK(hipDeviceSynchronize());
            auto round_ct = [&](float v) {
                if (h->es == 4) return v;
                uint32_t u; std::memcpy(&u, &v, 4);
                if ((u & 0x7fffffffu) > 0x7f800000u) return v;                       // NaN: compared as is
                u += 0x7fffu + ((u >> 16) & 1u); u &= 0xffff0000u;                   // round to nearest even, as the device conversion
                float r; std::memcpy(&r, &u, 4); return r;
            };
            auto elem = [&](const std::vector<unsigned char>& raw, size_t i) {
                float v;
                if (h->es == 2) { const uint32_t u = (uint32_t)reinterpret_cast<const uint16_t*>(raw.data())[i] << 16; std::memcpy(&v, &u, 4); }
                else v = reinterpret_cast<const float*>(raw.data())[i];
                return v;
            };
            float ew = 0.f, et = 0.f;
            int cnt = 0, worst = -1;
            auto check = [&](const Dense& d) {
                if (d.in <= 0 || d.out <= 0) return;
                std::vector<float> th((size_t)(d.in + 1) * d.ld);
                std::vector<unsigned char> w((size_t)(d.in + 1) * d.ldw * h->es), wt((size_t)d.out * d.ldt * h->es);
                HIP_OK(hipMemcpy(th.data(), (h->averaged ? h->ema_avg() : h->at<float>(h->off_theta)) + d.master, th.size() * 4, hipMemcpyDeviceToHost));
                HIP_OK(hipMemcpy(w.data(), h->at<void>(d.W), w.size(), hipMemcpyDeviceToHost));
                HIP_OK(hipMemcpy(wt.data(), h->at<void>(d.Wt), wt.size(), hipMemcpyDeviceToHost));
                float a = 0.f, b2 = 0.f;
                for (int r = 0; r <= d.in; ++r)
                    for (int c = 0; c < d.out; ++c) {
                        const float want = round_ct(th[(size_t)r * d.ld + c]);
                        a = std::max(a, std::fabs(elem(w, (size_t)r * d.ldw + c) - want));
                        b2 = std::max(b2, std::fabs(elem(wt, (size_t)c * d.ldt + r) - want));
                    }
                if (a > ew || b2 > et) worst = cnt;
                ew = std::max(ew, a); et = std::max(et, b2);
                ++cnt;
            };
            for (const Mod& md : h->mods) {
                for (const Dense& d : md.enc) check(d);
                check(md.head);
                for (const Dense& d : md.dec) check(d);
                check(md.outl);
                if (md.conv) { for (const ConvStage& st : md.cenc) check(st.d); for (const ConvStage& st : md.cdec) check(st.d); }
            }
            host_dst[0] = ew; host_dst[1] = et; host_dst[2] = (float)cnt; host_dst[3] = (float)worst;
            if (n_floats) *n_floats = 4;
            return;
        }
        else if (n == "grad_keep" || n == "grad_keep_masked") {
            // per captured step of the plan's training graphs, 16-step graph first, then the 4-step graph, then the single step:
            // 1 = the step stores its gradient (recorded by capture_steps).  "grad_keep": the plain plan, "grad_keep_masked": the masked one.
            const StepPlan& p = n == "grad_keep" ? h->plain : h->masked;
            if (!p.full.exec || !p.multi[0].exec || !p.multi[1].exec) throw Err("debug_fetch: the plan has no captured training graphs");
            for (const StepGraph* g : {&p.multi[0], &p.multi[1], &p.full}) {
                if (cnt + g->grad_keep.size() > max_floats) throw Err("debug_fetch: destination too small");
                for (unsigned char k : g->grad_keep) host_dst[cnt++] = (float)k;
            }
            if (n_floats) *n_floats = cnt;
            return;
        }
        else if (n == "ema_master") {       // the average as it lies in memory: P_int floats, master layout, padding included
            if (!h->ema_on) throw Err("debug_fetch: parameter averaging is off");
            src = h->ema_avg(); cnt = h->P_int;
        }
        else if (n.rfind("mulv", 0) == 0 || n.rfind("g0_", 0) == 0) {
            const bool g0 = n[0] == 'g';
            const int m = std::atoi(n.c_str() + (g0 ? 3 : 4));
            if (m < 0 || m >= h->M) throw Err("debug_fetch: modality out of range");
            src = h->at<void>(g0 ? h->mods[m].g0 : h->mods[m].mulv); cnt = g0 ? (size_t)h->B * 3 * h->ld_eps : (size_t)h->B * 2 * h->nz;
        } else throw Err("debug_fetch: unknown tensor " + n);
        if (cnt > max_floats) throw Err("debug_fetch: destination too small");
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(host_dst, src, cnt * 4, hipMemcpyDeviceToHost));
        if (n_floats) *n_floats = cnt;
    });
}

}  // extern "C"
