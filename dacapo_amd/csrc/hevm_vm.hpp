// HEVM virtual machine on the MI355X: state and host-side helpers behind the 18-symbol ABI of
// include/hevm_abi.h.  Mirrors struct SEAL_HEVM (/root/reference/lib/Runtime/SEAL_HEVM.cpp:15-402) with the
// SEAL objects replaced by HBM-resident limb arrays and HIP launches.
#pragma once
#include "wire_parse.hpp"
#include <algorithm>
#include <complex>
#include <deque>
#include <map>
#include <set>
#include <memory>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/hevm_abi.h"
#include "chacha.hpp"
#include "seal_serial.hpp"
#include "kernels.hpp"
#include "encoder.hpp"
#include "io_batch.hpp"
#include "plan.hpp"
#include "plan_flow.hpp"

namespace dacapo {

// Device allocations made on behalf of one VM, so that hevm_destroy (an extension: the reference's ABI never frees a VM) can return
// them.  The C ABI's entry points name the VM they act on (HEVM::enter); allocation sites call vm_malloc / vm_free instead of
// hipMalloc / hipFree.  Allocations made with no VM entered are not tracked (and live as long as the process, as before).
struct VmAllocs {
    std::unordered_set<void *> live;
};
extern thread_local VmAllocs *g_vm_allocs;
template <class T>
inline hipError_t vm_malloc(T **p, size_t bytes)
{
    const hipError_t e = hipMalloc((void **)p, bytes);
    if (e == hipSuccess && g_vm_allocs) g_vm_allocs->live.insert((void *)*p);
    return e;
}
inline hipError_t vm_free(void *p)
{
    if (p && g_vm_allocs) g_vm_allocs->live.erase(p);
    return hipFree(p);
}

// the wire structs (WireHeader, WireConfigBody, WireOp) and the two files' parsers live in a host-only TU: wire_parse.hpp

// CKKSEncoder restated on the host (encode/decode are untimed set-up work in the reference: SEAL_HEVM.cpp:242-267,
// :439-455); the RNS lift and every NTT run on the GPU.
class HostEncoder {
  public:
    HostEncoder(int logN);
    // values tiled over N/2 slots as src[i % len] (SEAL_HEVM.cpp:259-261); returns round(coefficients) as int128
    void encode(const double *src, size_t len, double scale, std::vector<__int128> &coeffs) const;
    // coeffs: N real coefficients already divided by the scale -> N/2 slot values (real parts)
    void decode(std::vector<std::complex<double>> &coeffs, double *out) const;
    size_t N, slots;
    int logN;
    const std::vector<std::complex<double>> &roots() const { return root_; }
    const std::vector<uint32_t> &slot_map() const { return slot_map_; }

  private:
    std::vector<std::complex<double>> root_; // exp(2 pi i bitrev(k) / 2N)
    std::vector<uint32_t> slot_map_;         // CKKSEncoder::matrix_reps_index_map_
};

struct Plain {
    u64 *d = nullptr;
    int level = 0;
    double scale = 1.0;
    bool arena = false; // d points into HEVM::plain_arenas (batched device encoder): not freed individually
    u64 *dsp = nullptr; // option hyb_double_hoist: the same plaintext's limbs over the special primes [ksp][N] (NTT form; in an arena), or null
};

struct KeySet {
    u64 *sk = nullptr;    // [K][N]
    u64 *pk = nullptr;    // [2][K][N]
    u64 *relin = nullptr; // [K-1][2][K][N]
    std::map<u32, u64 *> galois;
    // sparse-secret encapsulation (option boot_secret_hw > 0; opcode 20): swk_down switches s -> s' and exists only modulo q0 and the special
    // primes ([1][2][1 + ksp][N], the boot context's layout, HEVM::bctx); swk_up switches s' -> s over the whole chain ([digits][2][K][N]).
    // The ephemeral sparse secret s' itself is dropped as soon as both exist.
    u64 *swk_down = nullptr;
    u64 *swk_up = nullptr;
};

class HEVM {
  public:
    std::unique_ptr<Context> ctx;
    // sparse-secret encapsulation: the chain {q0, special primes} as a context of its own (a level-1 key switch of `ctx` is exactly a key switch
    // of this context), so that swk_down is stored over those 1 + ksp primes only and runs through the ordinary key-switch kernels
    std::unique_ptr<Context> bctx;
    void ensure_boot_context();
    std::unique_ptr<HostEncoder> encoder;
    KeySet keys;
    bool debug = false;
    void *ckks_handle = nullptr; // dc_context* handed out by hevm_context()
    RngKeys rng;          // ChaCha20 keys of this VM's randomness (chacha.hpp)
    u64 enc_counter = 0;  // encryptions made so far: the `object` of the next one
    u64 *d_epoch = nullptr; // run() counter in HBM, mixed into the encryption randomness (graph replays stay fresh)

    // The VM's HIP stream and the scratch of one in-flight composite op.  run() executes the batched plan (plan.hpp); with
    // option plan = 0 or setDebug(true) it is the reference's loop instead: one instruction at a time, in program order.
    struct Lane {
        hipStream_t stream = nullptr;
        Workspace ws;
        Plain boot_plain; // staging plaintext of opcode 10
    };
    std::vector<Lane> lanes; // one entry
    int cur = 0;
    hipStream_t S() const { return lanes[cur].stream; }
    const Workspace &W() const { return lanes[cur].ws; }
    void execute();
    void dispatch(const WireOp &op);

    // program
    std::vector<std::vector<double>> buffer; // constants of the .cst file
    // batched device encoder (encoder.hip): tables, and the arenas the plaintext registers of the loaded program live in
    EncTables enc_tables;
    std::vector<u64 *> plain_arenas;
    // option online_encode = 1: plaintexts are encoded at use from the resident constants instead of being kept pre-encoded
    bool online_encode = false;
    struct OnlineEncode {
        double *d_consts = nullptr;
        size_t const_bytes = 0;
        std::map<int, EncItem> items; // plaintext register -> what to encode
    } online;
    bool host_encoder = false; // option host_encoder = 1: encode on the host (HostEncoder), one plaintext at a time
    void ensure_enc_tables();
    void preprocess_device();
    void free_plains();
    WireHeader header{};
    WireConfigBody config{};
    std::vector<WireOp> ops;
    std::vector<uint64_t> arg_scale, arg_level, res_scale, res_level, res_dst;
    std::deque<hevm_ctxt> ciphers; // deque: growing it never invalidates references to registers
    std::vector<Plain> plains;

    // device CRT tables per level + staging plaintext of opcode 10
    struct CrtTables {
        u64 *inv, *mmod, *hmod, *hdig;
        double *mdbl;
    };
    std::map<int, CrtTables> crt_;
    const CrtTables &crt_tables(int ell);

    // ---- batched plan (plan.hpp): built on the first run() of a loaded program -----------------------------
    enum PopKind { P_ROT, P_MULCC, P_RESCALE, P_SUM, P_NEG, P_MULP, P_ADDP, P_COPY, P_BOOT, P_MODRAISE, P_ROTSUM, P_MULSUM };
    static constexpr int kPopKinds = 12;
    // A step by its kind alone: name in traces; heavy = key switch, rescale or opcode 10: max_batch items to a step where limb-wise kinds take 4096
    // (step_chunk); launches of one step as the trace's "step launches" and the levelling pass count them (not the ~launches estimate that gates capture)
    struct KindTraits { const char *name; bool heavy; int launches; };
    static constexpr KindTraits kKind[kPopKinds] = { { "rot", true, 5 },  { "mulcc", true, 5 }, { "rescale", true, 3 }, { "sum", false, 1 },      { "neg", false, 1 },   { "mulp", false, 1 },
                                                     { "addp", false, 1 }, { "copy", false, 1 }, { "boot", true, 4 },    { "modraise", false, 1 }, { "rotsum", true, 5 }, { "mulsum", true, 5 } };
    size_t step_chunk(PopKind k) const { return std::max<size_t>(1, (kKind[k].heavy ? (size_t)max_batch : (size_t)4096) / (size_t)streams); } // pseudo-ops per step
    struct Val {
        int level = 0;
        double scale = 1.0;
        int root = -1;     // value whose buffer this one aliases (modswitch = a view with fewer limbs)
        int def_step = -1; // step producing it (-1: program input)
        int last_use = -1; // last step reading it
        int uses = 0;
        int def_pop = -1;
        u64 *buf = nullptr;
        bool external = false, pinned = false;
    };
    struct Pop {
        PopKind kind;
        int level = 0;
        int dst = -1;
        std::vector<int> srcs;
        std::vector<int> src_plain; // P_SUM: plain register multiplying srcs[k], or -1
        u32 elt = 0;
        const u64 *key = nullptr;
        int plain = -1, target_level = 0;
        int rot = 0; // P_ROT: 1 a hop of a rotate / conj instruction, 2 the same on the hoisted path (option ks_hoist; target_level = -2: a bucket of its own); 0 opcode 20's switch
        int rs_add = -1, rs_mul = -1; // P_RESCALE: plain registers of a folded addcp / mulcp (operand = (srcs + add) * mul)
        bool rs_sum = false;          // P_RESCALE: srcs/src_plain are the terms of a folded n-ary sum
        int boot_drop = -1;           // P_BOOT: prime index of a folded rescale (operand read before the division), or -1
        double boot_src_scale = 0.0;  // P_BOOT with boot_drop: scale of the folded rescale's result
        bool dead = false;
        int wave = 0, step = -1;
        // lazy sums (option hyb_lazy_sum): a P_ROT remembers the instruction it came from and whether it is that instruction's LAST hop;
        // a P_ROTSUM (dst = sum of galois_{elts[k]}(srcs[k]) with one division by P, plan.hpp hyb_rotate_sum) lists its rotations
        int op = -1;
        bool direct = false;
        std::vector<u32> elts;
        std::vector<const u64 *> keys;
        std::vector<int> ops;
        // a P_MULSUM (option ks_lazy_relin: dst = relin(sum_k signs[k] srcs[2k] (x) srcs[2k + 1]), plan.hpp b_mul_sum_relin) lists its products: ops[k]
        // the mulcc instruction, op the addcc / negate instruction whose result it computes
        std::vector<int> signs;
        // option ks_flatten_sums: a hop of a rotate instruction remembers the value the INSTRUCTION rotates (inst_src) and the instruction's first
        // hop (first_hop: a pop index; the hops of one instruction are adjacent); a P_ROTSUM that stands for a stage of a rotate-and-add chain
        // (plan_flatten.hpp) adds `addend` exactly in its inner-product launch and lists the stage's hops and its members' slot offsets:
        // flat_ops = (rotate instruction, addcc instruction) per hop, op = the closing addcc
        int inst_src = -1, first_hop = -1, addend = -1;
        std::vector<int> flat_ops, flat_offsets;
        std::vector<int> plains; // P_ROTSUM, option hyb_double_hoist: the plaintext register multiplying rotation k before it joins the sum, or -1
    };
    struct Step {
        PopKind kind;
        int level = 0, first = 0, count = 0; // range in the kind's device item table
        int target = 0;                     // P_BOOT: primes of the result
        int wave = 0, lane = 0;             // steps of one wave are independent: lane 1 runs on the auxiliary stream
        Handoff h;                          // link to a fused producer (h.in) / consumer (h.cont, h.out) step, plan.hpp
        int fused_consumer = -1;            // index of the step whose first phase this step's last kernel computes
        bool fold_rs = false;               // P_MULCC, option ks_fold_rescale: every item also does the rescale that alone reads it (first: in d_mulrs);
                                            // those rescales are in no step of their own, and the step defines THEIR results
        int gfirst = 0, gcount = 0;         // P_SUM: the step's items as groups that share sources (plan.hpp SumGroup), when it runs that way; P_ROTSUM: its groups (in d_ks; option ks_lazy_sum: the distinct sources' items follow them)
        bool addend = false;                // P_ROTSUM, option ks_flatten_sums: the groups' src fields are addends (or null), plan.hpp hoist_rotate_sum
        int unique = 0;                     // P_ROT, grouped-digit mode: distinct source ciphertexts among the items (shared decompositions)
                                            // ... and option ks_hoist (target == -2): the same count; d_ks[gfirst .. gfirst + unique) are the sources' items
        // what the step's launches read and write, by pool buffer (a value and its modswitch views share one): the edges of the explicitly
        // built graph (option plan_graph = 2, capture_plan_dag)
        std::vector<const u64 *> reads, writes;
    };
    // The device memory a plan allocates for itself (item tables, arenas, the links' first-phase buffers, both lanes' scratch) comes from plan_alloc, which
    // lists it in `owned`; release_plan frees that list and resets everything but pool and events.  The typed pointers below are read, never freed.
    struct Plan {
        bool ready = false;
        std::vector<void *> owned;
        std::vector<Val> vals;
        std::vector<Pop> pops;
        std::vector<Step> steps;
        std::vector<int> final_val; // architectural register -> value at program end
        KsItem *d_ks = nullptr;
        MulItem *d_mul = nullptr;
        MulSumItem *d_mulsum = nullptr;      // option ks_lazy_relin: the P_MULSUM steps' items ...
        MulTerm *d_mulsum_terms = nullptr;   // ... and their terms
        MulRsItem *d_mulrs = nullptr;        // items of the multiply steps whose rescale is folded in (Step::fold_rs)
        RsItem *d_rs = nullptr;
        EwItem *d_ew = nullptr;
        SumItem *d_sum = nullptr;
        SumSrc *d_sum_srcs = nullptr;
        SumGroup *d_sumg = nullptr;
        SumGroupSrc *d_sumg_srcs = nullptr;
        CtView *d_cont_other = nullptr;      // CONT_MUL links: the consumers' other operands
        // on-line encode: per wave, the plaintext registers first read in it, encoded into a window recycled at wave granularity
        struct EncGroup { int wave, level, first, count; u64 *out; };
        std::vector<EncGroup> enc_groups;
        EncItem *d_enc_items = nullptr;
        u64 *enc_arena = nullptr;
        double2 *enc_scratch = nullptr;
        int *d_enc_overflow = nullptr;
        size_t enc_arena_bytes = 0, enc_scratch_bytes = 0;
        std::vector<EwItem> h_ew;            // host copy of the elementwise item table (modraise launches its NTTs per item)
        size_t n_fused = 0;
        // opcode 10: item table, the divide-and-round items of the zero-encryptions, the zero-encryption arena and scratch
        BootItem *d_boot = nullptr;
        RsItem *d_boot_rs = nullptr;         // (option zenc_head = 0)
        ZencItem *d_boot_zenc = nullptr;     // (option zenc_head = 1)
        size_t zenc_bytes = 0;
        u64 *zenc = nullptr, *boot_ue = nullptr, *boot_tmp = nullptr, *boot_pt[2] = { nullptr, nullptr }, *boot_ptx[2] = { nullptr, nullptr };
        signed char *boot_e = nullptr; // option zenc_head = 1: the noise polynomials of a chunk, [chunk][2][N] bytes at the end of boot_ue (which then holds u alone; no boot_tmp)
        struct BootChunk { int first, count, target; };
        std::vector<BootChunk> boot_chunks; // zero-encryption launches at the start of every run
        BatchWs ws[2]; // per lane
        std::vector<hipEvent_t> events; // fork/join pairs of the waves that use the auxiliary stream
        std::vector<u64 *> pool; // every pool buffer ever allocated (reused across plans)
        int64_t n_keyswitch = 0, n_ntt = 0;
        int64_t n_hops = 0, n_decomp = 0; // rotation hops and the decompositions computed for them (hevm_last_run_hoist_stats)
        int64_t n_relin_groups = 0, n_relin_products = 0; // P_MULSUM items and their terms (hevm_last_run_relin_stats)
        int64_t n_flat_groups = 0, n_flat_members = 0, n_flat_hops = 0; // flattened stages, their rotations and the hops they absorbed, once per stream (hevm_last_run_flatten_stats)
        int64_t n_add_folds = 0;          // two-term sums that a rotation's last hop computes (option ks_fold_add; hevm_last_run_add_fold_stats), per stream until the plan is ready
        int64_t n_fold = 0;               // items of multiply steps that run with their rescale folded in (hevm_last_run_fold_rescale_stats)
        size_t launches = 0, max_live = 0;
        hipGraph_t graph = nullptr;
        hipGraphExec_t graph_exec = nullptr;
    } plan;
    bool plan_graph = true; // replay the plan's launch sequence as one HIP graph (option plan_graph = 0: issue it launch by launch)
    bool plan_dag = false;  // option plan_graph = 2: the graph is BUILT from the plan's own dependencies instead of captured from two streams
    void capture_plan();
    bool capture_plan_dag();
    void issue_step(const Step &st, hipStream_t q);
    void drop_plan_graph();
    void *plan_alloc(size_t bytes);
    void release_plan();
    void issue_head(hipStream_t s);
    void issue_plan(hipStream_t s);
    bool use_plan = true;
    bool test_zero_enc = false; // hevm_test_zero_encryption: encryptions of zero are (0, 0) -- INSECURE, parity tests of opcode 10 only
    int max_batch = 64; // items per heavy step (option max_batch): 64 measured best on the ResNet-20 program (16 ... 256 tried)
    std::vector<u64 *> home; // permanent buffer block of every architectural register (program inputs live here)
    // Throughput mode: `streams` independent ciphertext streams share the program, keys and plaintexts; every buffer is a
    // block of `streams` slices and encrypt/decrypt/getCtxt address the slice selected by hevm_select_stream().
    int streams = 1, sel = 0;
    std::vector<u64 *> reg_base; // base of the block currently holding each architectural register
    void set_streams(int n);
    void select_stream(int s);
    void build_plan();
    // leaves of build_plan: they read the finished values, pops and steps and write Plan fields (and, on-line encode, where a plaintext lies)
    CtView plan_view(int v, int stream) const;
    const u64 *plain_ptr(int reg) const { return reg >= 0 ? plains.at((size_t)reg).d : nullptr; }
    std::pair<int, int> push_terms(std::vector<SumSrc> &h_srcs, const Pop &p, int stream) const;
    void place_online_encode(const std::vector<std::vector<int>> &step_pops);
    void build_boot_tables(const std::vector<std::pair<int, int>> &boot_pops, int boot_tmax, size_t need_bpt, size_t need_bptx, std::vector<SumSrc> &h_srcs, size_t &need_d, size_t &need_m);
    void report_plan(const double (&sum_stat)[5], int max_wave, int levels_moved) const;
    void run_plan();
    void boot_item(CtView src, int src_level, double src_scale, hevm_ctxt &dst, int target_level);
    void plan_zero_encrypt(int first, int B, int t, hipStream_t s);
    void plan_boot_step(int first, int B, int ell, int t, int lane, hipStream_t s, const Handoff &h);
    bool rot_compose = false; // option rot_compose: rotations without a direct key are the shortest sum of offsets that have one (HEVM::compose_rotation)
    std::vector<int> compose_rotation(int steps) const;
    mutable std::vector<int> rot_offsets;   // offsets with a key, in the search order; rebuilt when the key set changes
    mutable std::set<int> rot_offset_set;
    mutable size_t rot_offsets_epoch = (size_t)-1;
    int boot_secret_weight = 0; // option boot_secret_hw = h': key generation also draws an ephemeral secret of weight h' and the two switching keys
    int secret_weight = 0; // option secret_hw = h: key generation draws a ternary secret with exactly h non-zero coefficients (0: uniform ternary, SEAL's)
    // option ks_hoist = 1 (SEAL-layout keys): every rotation hop takes c1's digits BEFORE the automorphism (hoist_ks.hip), and the hops of a
    // plan step that read one source share its decomposition.  Changes the rounding: off by default.
    bool ks_hoist = false;
    // option ks_lazy_sum (with ks_hoist): 1 sums of bare rotations share one division by P, 2 rotations times a plaintext join them too
    // (plan_exec.hip section 2b; hoist_ks.hip hoist_rotate_sum)
    int ks_lazy = 0;
    // option ks_fold_rescale = 1 (SEAL-layout keys): a multiply and the rescale that alone reads it run as one step
    // (plan_exec.hip section 4; plan.hpp b_mul_relin_rescale).  Every limb equals the default path's.
    bool ks_fold_rescale = false;
    // option ks_lazy_relin = 1 (SEAL-layout keys): sums of single-use ct x ct products are relinearised once (plan_exec.hip section 1b;
    // plan_relin.hpp names the groups, plan.hpp b_mul_sum_relin runs them).  Changes the rounding: off by default.
    bool ks_lazy_relin = false;
    // option ks_flatten_sums = f (2 .. 6; with ks_hoist and ks_lazy_sum): stages of up to f hops of a rotate-and-add chain run as one hoisted lazy
    // sum with an addend (plan_exec.hip section 1a; plan_flatten.hpp names the groups).  Changes the rounding: off by default.
    int ks_flatten = 0;
    // option ks_fold_add = 1 (SEAL-layout keys): y + rotate(x, o) is the rotation's own last hop with y as its addend (plan_exec.hip section 3a;
    // plan.hpp KsItem::add).  Every limb equals the default path's.  The loop (plan = 0) runs the instructions as written.
    bool ks_fold_add = true;
    PlanFlow program_flow() const; // the loaded program's dataflow under the result registers of this moment (plan_flow.hpp)
    std::vector<FlattenGroup> flatten_groups(const PlanFlow &flow, bool every_key) const; // the program's groups under the key set held (every_key: as if every offset had a key)
    // option zenc_head = 1: the zero-encryptions at the start of a plan's run() transform only u (plan_zero_encrypt).  Every limb equals
    // zenc_head = 0's.  zenc_chunk_hook (hooks build, test_hooks.hip: HEVM_TEST_ZENC_CHUNK): items per chunk of that head instead of kZencChunk, 0 = unset
    bool zenc_head = true;
    static constexpr int kZencChunk = 64;  // items per chunk of that head (measured: profiles/zenc_head_ab.txt)
    int zenc_chunk_hook = 0;
    KsItem *d_hoist_items = nullptr; // the loop's (plan = 0) two-entry item table: the hop and its source
    void rotate_hop_vm(CtView dst, CtView src, u32 elt, const u64 *key, int ell);
    bool chain_fusion = true; // option chain_fusion = 0: every step runs all of its own launches
    hipStream_t aux_stream = nullptr;
    // option hyb_double_hoist = 1 (with hyb_lazy_sum): rotations multiplied by a plaintext join the lazy sums; the plaintexts' special-prime limbs
    // are encoded when the plan first names them (the program's constants and encode items stay resident for that)
    bool double_hoist = false;
    double *dh_consts = nullptr;
    std::map<int, EncItem> dh_items; // plaintext register -> its encode item (preprocess_device)
    void ensure_special_limbs(const std::vector<int> &plain_regs);
    bool lazy_sums = false; // option hyb_lazy_sum = 1: sums of direct-key rotations share one division by P (plan_exec.hip section 2b)
    bool fold_rescale_into_boot = false; // option fold_rescale_boot = 1: do a rescale that only feeds an opcode 10 inside its re-encoder
    int plan_lanes = 2; // independent steps of a wave also use an auxiliary stream (pays off only inside the graph; option plan_lanes = 1: one stream)
    // option plan_level: 0 the plan levels its operations ASAP; 1 slack-aware levelling (plan_levels.hpp) and a plaintext addend hoisted out of a
    // rescale's folded sum (plan_exec.hip section 2); 2 the hoist alone (a measurement leg).  Every limb is the same under all three
    int plan_level = 1;
    void bump_epoch(hipStream_t s);

    // statistics of the last run()
    int64_t op_counts[11] = { 0 };
    int64_t n_keyswitch = 0, n_ntt = 0;
    int64_t n_hops = 0, n_decomp = 0; // hevm_last_run_hoist_stats
    int64_t n_fold = 0;               // hevm_last_run_fold_rescale_stats
    int64_t n_add_folds = 0;          // hevm_last_run_add_fold_stats
    int64_t n_relin_groups = 0, n_relin_products = 0; // hevm_last_run_relin_stats
    int64_t n_flat_groups = 0, n_flat_members = 0, n_flat_hops = 0; // hevm_last_run_flatten_stats
    double t_bootstrap = 0.0; // host wall time spent inside opcode 10

    VmAllocs allocs;   // device memory held by this VM (hevm_destroy)
    HEVM() { g_vm_allocs = &allocs; }
    void destroy_device_state(); // streams, events, graph, every tracked allocation; the object is unusable afterwards
    size_t key_elems() const { return (size_t)ctx->key_digits() * 2 * ctx->K * ctx->N; }
    void init_context(int logN, int K, const u64 *primes, int dir_ksp = 0, int dir_alpha = 0);
    void generate_keys(const RngKeys &rng, bool secret, bool pub, bool eval);
    void gen_kswitch_key(u64 *key, const u64 *new_key, u64 key_id);
    void gen_kswitch_key_in(Context &c, u64 *key, const u64 *key_sk, const u64 *new_key, u64 key_id); // key under key_sk for new_key, in context c
    void fill_sparse_secret(u64 *dst, int weight, u32 domain);   // [K][N] coefficient form: exactly `weight` coefficients +-1
    void generate_boot_switch_keys();
    size_t swk_down_elems() const { return (size_t)2 * (1 + ctx->ksp) * ctx->N; }
    void add_galois_key(u32 elt);
    void save_keys(const std::string &dir);
    void load_keys(const std::string &dir, bool need_secret, bool need_public, bool need_eval);
    sealio::ParmsId parms_id_at(int limbs) const; // SEAL parms_id of the chain truncated to `limbs` primes (limbs = K: key level)
    sealio::ParmsId boot_parms_id() const { return sealio::parms_id(bctx->N, bctx->primes.data(), (size_t)bctx->K); } // {q0, special primes}
    void save_ctxt(size_t reg, const std::string &path);
    void load_ctxt(size_t reg, const std::string &path);

    void load_constants(const void *data, size_t len);
    void load_program(const void *data, size_t len, bool header_only);
    void reset_res_dst();
    void preprocess();
    void encode_internal(Plain &dst, const double *src, size_t len, int level, int scale_bits);
    hevm_ctxt &reg(size_t i);
    void encrypt_plain(hevm_ctxt &dst, const Plain &pt);
    void encrypt(int64_t i, const double *dat, int len);
    void decrypt(int64_t i, double *out);
    // limbs a register at `level` is decoded from (decrypt and decrypt_batch: the device CRT composes at most 16, see decrypt)
    int decode_limbs(int level) const { return !host_encoder && level > 16 ? 16 : level; }

    // ---- batched encrypt / decrypt (hevm_encrypt_batch / hevm_decrypt_batch): `count` streams' inputs or results as ONE launch sequence and
    // one synchronisation, values in host (where = 0) or device (where = 1) memory.  Limbs and doubles equal `count` calls of encrypt /
    // decrypt on those streams in ascending order.  The launches per chunk do not depend on the number of items in it (but for the
    // transform's own form, kernels.hpp launch_ntt: one launch or two by its limb count at N = 2^15).
    // Scratch is the VM's own (a client VM has no plan to borrow from): one block per direction, allocated on first use and grown when a call
    // needs more.  Chunk rule: io_chunk(per_item) = min(kIoChunk, max(1, kIoScratchBytes / per_item)) items per pass of the sequence, per_item
    // being the bytes one item needs at the call's level -- so a block is at most max(kIoScratchBytes, one item): at N = 2^17 with 31
    // primes an encryption at level 30 needs 126 MiB (limbs of 1 MiB: u over 31 primes, plaintext 30, divide-and-round 62, encoder 2.5, noise
    // 0.25), 8 items to a chunk, 1 GiB; a decryption 18.5 MiB (16 limbs at most, the FFT's 2, the slots' 0.5).  Chunks reuse the block in stream order.
    static constexpr int kIoChunk = 32;
    static constexpr size_t kIoScratchBytes = (size_t)1 << 30;
    struct IoBatch {
        u64 *enc = nullptr, *dec = nullptr; // the two scratch blocks
        size_t enc_bytes = 0, dec_bytes = 0;
        void *tab = nullptr;                // device item tables of the call in flight
        size_t tab_bytes = 0;
        std::vector<unsigned char> h_tab;   // their host image (lives until the next call: the upload is asynchronous)
        int *d_overflow = nullptr;          // the encoder's "coefficient does not fit" flag
        int64_t launches = 0, chunks = 0;   // hevm_last_io_stats: kernel launches and chunks of the last batch call
    } io;
    int io_chunk(size_t per_item_bytes) const { return (int)std::min<size_t>((size_t)kIoChunk, std::max<size_t>(1, kIoScratchBytes / per_item_bytes)); }
    void io_check_streams(const char *what, int first_stream, int count) const;
    void io_reserve(u64 *&block, size_t &have, size_t bytes);
    void *io_upload_tables(size_t bytes);
    void encrypt_batch(int64_t arg, const double *vals, int len, int64_t stride, int first_stream, int count, int where);
    void decrypt_batch(int64_t reg, double *out, int64_t stride, int first_stream, int count, int where);
    int phase_batch(int64_t reg, u64 *out_dev, int64_t stride, int first_stream, int count);
    void run();

    // opcode handlers (SEAL_HEVM.cpp:268-334)
    void op_rotate(int dst, int src, int offset);
    void op_negate(int dst, int src);
    void op_rescale(int dst, int src);
    void op_modswitch(int dst, int src, int down);
    void op_addcc(int dst, int lhs, int rhs);
    void op_addcp(int dst, int lhs, int rhs);
    void op_mulcc(int dst, int lhs, int rhs);
    void op_mulcp(int dst, int lhs, int rhs);
    void op_bootstrap(int dst, int src, int target_level);
    void op_conj(int dst, int src);
    void op_modraise(int dst, int src, int target);
    void op_setscale(int dst, int src, int const_idx);
    void op_keyswitch(int dst, int src, int which);
    std::vector<u32> rotate_hops(int steps) const;

    CtView view(const hevm_ctxt &c) const { return CtView{ c.data, (long)c.poly_stride }; }
};

} // namespace dacapo
