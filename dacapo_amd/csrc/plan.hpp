// Batched execution plan of an HEVM program.
//
// The reference interprets the bytecode one blocking SEAL call at a time (SEAL_HEVM.cpp:336-401).  On the MI355X a
// single low-level ciphertext op (2-5 primes) is a few microseconds of work spread over a dozen dependent launches:
// issued one by one the GPU idles between them.  HBM is plentiful (288 GB), so run() instead executes a PLAN
// built once per loaded program:
//   1. registers are renamed (SSA): every op result gets its own buffer from a pool, which removes the WAR/WAW
//      hazards that ReuseBuffer.cpp's register recycling introduces and leaves only true dataflow;
//   2. ops are levelled by dataflow depth ("waves"); all ops of one kind and level in a wave become ONE batched
//      launch sequence (the key switches of the ~100 independent rotations of a convolution run as one batch);
//   3. chains of ct+ct additions are summed by one n-ary kernel -- modular addition is exact, so the result limbs
//      are bit-identical to the sequential chain.
// Every kernel takes a device-resident table of per-item views; level/scale bookkeeping is resolved at plan time.
#pragma once
#include "crt_device.hpp"
#include "kernels.hpp"

namespace dacapo {

struct KsItem {   // one key-switch hop of a rotation: dst = apply_galois(src)
    CtView src, dst;
    const u64 *key;
    u32 elt;
    u32 slot;     // grouped-digit mode: which decomposition of the batch this hop reads (hops of one source ciphertext share one); else 0
    // double hoisting (option hyb_double_hoist; items of a lazy sum only): the plaintext that multiplies this rotation's result before it joins
    // the sum -- its limbs over the data primes [level][N] and over the special primes [ksp][N] (both NTT form) -- or null
    const u64 *plain = nullptr, *plain_sp = nullptr;
    // option ks_fold_add (dc_ct_rotate_hop_add): dst = apply_galois(src) + add, add a ciphertext at the hop's level that the fused middle puts
    // into its accumulators' start values (fused_ks.hip f_ks_frows_mac_kernel) -- exact, no launch of its own; p == nullptr: no addend.  It may
    // be src or dst.  Only b_rotate_hops on SEAL-layout keys with the fused middle reads it (it aborts where the middle is not fused); the
    // grouped-digit, hoisted and lazy-sum kernels ignore it
    CtView add = CtView{ nullptr, 0 };
};
struct MulItem {  // dst = relinearize(a * b)
    CtView a, b, dst;
};
// dst (level l - 1) = rescale_to_next(((relinearize(a * b) + add on c0) * mul)) with the rescale folded into the key switch (option
// ks_fold_rescale; fused_ks.hip f_dr2_icols_lift_fcols_kernel).  mul is a CONSTANT polynomial: limb i's value is mul[i * mul_stride]
// (a plaintext [level][N] whose every value of a limb equals its first: stride N; a table of residues: stride 1), or null
struct MulRsItem : MulItem {
    const u64 *add = nullptr; // plaintext [level][N] added to c0, or null
    const u64 *mul = nullptr;
    long mul_stride = 0;
};
// dst = relinearize(sum of `count` signed tensor products terms[first ...]) with ONE key switch (dc_ct_mul_sum_relin; fused_ks.hip
// f_irows_tensor_sum_kernel / f_frows_sum_final_kernel).  The three-part sum is formed in exact modular arithmetic, so c0, c1 and the key-switch
// target equal Oracle.tensor per term + poly_add / poly_sub; the rounding is that of one mod-down instead of `count`.
struct MulTerm {  // sign * (a (x) b)
    CtView a, b;
    int sign;     // +1 or -1
};
struct MulSumItem {
    CtView dst;
    int first, count; // 1 <= count <= kMulSumMax
};
// The cap bounds the dependent walk (table entry -> pointers -> limbs, one round trip per term) that the first and the last kernel of the key
// switch make per tile; the accumulators themselves fold every 8 terms and hold any count (fused_ks.hip tensor_sum).
constexpr int kMulSumMax = 32;
struct RsItem {   // dst = rescale_to_next(expr), expr = ((src | sum of `count` terms srcs[first ...]) + add on c0) * mul
    CtView src, dst;
    int first = 0, count = 0;          // count == 0: expr starts from src
    const u64 *add = nullptr;          // plaintext [level][N] added to c0 (a single-use addcp folded in), or null
    const u64 *mul = nullptr;          // plaintext multiplying both polys (a single-use mulcp folded in), or null
};
struct ZencItem { // dst = rescale_to_next(pk * u + e): one zero-encryption of a plan (hevm_vm.hip plan_zero_encrypt, option zenc_head = 1)
    const u64 *u;  // NTT(u) over the target's primes and the dropped one, [t + 1][N]; pk and e are the launch's (one key, e by position)
    CtView dst;
};
struct EwItem {   // dst = a (op) b ; plaintext operand: b.p = limbs, b.poly_stride = 0
    CtView dst, a, b;
};
struct SumSrc {   // one term of a sum: a ciphertext, optionally times a plaintext (a ct*pt product folded into the sum)
    CtView v;
    const u64 *plain; // [level][N] or null
};
struct SumItem {  // dst = sum of `count` terms srcs[first ...]
    CtView dst;
    int first, count;
};

// n-ary sums of one step that name the same ciphertexts, run together (batch_ops.hip b_sum_group_kernel): up to kSumGroup items to a thread,
// the union of their sources walked once -- a rotated ciphertext that feeds 8 output channels of a convolution, or 8 giant steps of a
// matrix-vector product, is read once instead of 8 times.
constexpr int kSumGroup = 8;
struct SumGroupSrc { // one source of a group and, per item, what multiplies it
    CtView v;
    const u64 *plain[kSumGroup]; // [level][N]; null: the item does not use this source; kSumAddOnly: the item adds it as it is
};
struct SumGroup {
    CtView dst[kSumGroup];
    int first, count, items; // sources gsrcs[first ... first + count), items <= kSumGroup
};
__host__ __device__ inline const u64 *sum_add_only() { return reinterpret_cast<const u64 *>((uintptr_t)8); }

struct BootItem { // opcode 10: dst = Enc(re-encode(Dec(src))) = zenc + (plaintext, 0)
    CtView src, dst;
    const u64 *zenc; // fresh public-key encryption of zero at the target level, [2][t][N], made at the start of the run
    double ratio;    // new_scale / old_scale (divided by the dropped prime when a rescale has been folded in, see plan_exec.hip)
    // operand expression like RsItem's: ((src | sum of `count` terms) + add on c0) * mul, decrypted in the first loader
    int first = 0, count = 0;
    const u64 *add = nullptr, *mul = nullptr;
};

// A step's link to a fused neighbour.  The last kernel of every composite op is a forward ROWS phase and the first kernel of
// every composite op an inverse ROWS phase over the SAME tiles (ntt_tile.hpp: the last pass of one and the first pass of the
// other use the same thread <-> coefficient map).  When the plan sees that step B only consumes what step A produces, A's last
// kernel keeps going: it stores its result, forms B's first-phase operand from the values still in registers and runs B's
// inverse ROWS phase, writing B's first-phase buffer -- one launch (and one trip through HBM) fewer per link.
enum ContKind : int {
    CONT_NONE = 0,
    CONT_RS = 1,   // consumer is a rescale: inverse phase of the limb it drops (both polynomials)
    CONT_MUL = 2,  // consumer is a ct x ct multiply: inverse phase of out.c1 * other.c1 (the tensor product's c2), every limb
    CONT_BOOT = 3, // consumer is an opcode 10: inverse phase of out.c0 + out.c1 * s (Decryptor::decrypt), every limb
};
struct Handoff {
    int cont = CONT_NONE;          // what this step's last kernel also computes ...
    u64 *out = nullptr;            // ... into the consumer's first-phase buffer ([B][2][N], [B][l][N], [B][l][N])
    const CtView *other = nullptr; // CONT_MUL: device table [B] of the consumer's other operand (p == nullptr: a square)
    const struct RsItem *rs_items = nullptr; // CONT_RS: the consumer's items (a "+ plaintext" / "* plaintext" folded into it applies first)
    const u64 *sk = nullptr;       // CONT_BOOT: secret key [K][N]
    const u64 *in = nullptr;       // this step's own first phase was computed by its producer: read it here instead of launching it
};

// scratch of one batched step, sized for the largest batch of the plan
struct BatchWs {
    u64 *target = nullptr; // [B][l][N]     key-switch target, NTT form
    u64 *digits = nullptr; // [B][l][N]     its coefficient-domain digits (rescale: [B][2][N] dropped limbs)
    u64 *ext = nullptr;    // [B][l*l][N]   digits lifted to the other moduli
    u64 *acc = nullptr;    // [B][2][l+1][N]
    u64 *tmp = nullptr;    // [B][2][l][N]
};

// `unique`: grouped-digit mode only -- the number of distinct decompositions the items' `slot` fields name (0: every item its own)
// `addend`: some item carries one (KsItem::add); aborts unless the batch runs the fused middle on SEAL-layout keys, which alone adds it
void b_rotate_hops(Context &c, const BatchWs &w, const KsItem *d_items, int B, int ell, hipStream_t s, const Handoff &h = Handoff{}, int unique = 0,
                   bool addend = false);
void b_mul_relin(Context &c, const BatchWs &w, const MulItem *d_items, const u64 *relin_key, int B, int ell, hipStream_t s,
                 const Handoff &h = Handoff{});
// a multiply and the rescale that alone reads it as ONE five-launch sequence (SEAL-layout keys, the latency-shaped launch forms only:
// mul_relin_rescale_fused says whether a batch of B at level ell has it; otherwise run b_mul_relin and b_rescale -- the limbs are the same).
// h.in as for b_mul_relin; h.cont CONT_MUL / CONT_BOOT as for b_rescale.
bool mul_relin_rescale_fused(const Context &c, int B, int ell);
void b_mul_relin_rescale(Context &c, const BatchWs &w, const MulRsItem *d_items, const u64 *relin_key, int B, int ell, hipStream_t s,
                         const Handoff &h = Handoff{});
void b_rescale(Context &c, const BatchWs &w, const RsItem *d_items, int B, int ell, hipStream_t s, const SumSrc *d_srcs = nullptr,
               const Handoff &h = Handoff{});
// B sums of signed ct x ct products, each relinearised by ONE key switch: b_mul_relin's launch sequence (same count, same middle) with the
// term-walking first and last kernels.  SEAL-layout keys only (aborts otherwise).  No destination may be an operand of the batch.
void b_mul_sum_relin(Context &c, const BatchWs &w, const MulSumItem *d_items, const MulTerm *d_terms, const u64 *relin_key, int B, int ell,
                     hipStream_t s);
// hoisted rotations on SEAL-layout keys (hoist_ks.hip; option ks_hoist, dc_ct_rotate_hoisted): B hops over U <= B decompositions, digits taken
// BEFORE the automorphism (oracle orc_rotate_ks_hybrid at one special prime).  d_items[b].slot indexes d_sources[0 .. U): items with the
// identity element whose src is the source ciphertext.  w is sized as for B default hops.
void hoist_rotate_hops(Context &c, const BatchWs &w, const KsItem *d_items, const KsItem *d_sources, int B, int U, int ell, hipStream_t s);
// lazy sums on the same decompositions (option ks_lazy_sum, dc_ct_rotate_sum_hoisted): G sums of B members, ONE division by P per sum (oracle
// orc_rotate_acc_hybrid per member, Oracle.lazy_mul_plain / lazy_add, one orc_moddown_hybrid per group).  d_groups[g] as for hyb_rotate_sum:
// dst, elt = first member, slot = member count; a member's plain / plain_sp ([level][N] / [1][N]) multiply it in the raised basis, or null.
// addend (dc_ct_rotate_sum_hoisted_add, option ks_flatten_sums): d_groups[g].src is a ciphertext at level ell added to sum g exactly, with no
// launch of its own (src.p == nullptr: that group has none); it may be a source or a destination of the batch
void hoist_rotate_sum(Context &c, const BatchWs &w, const KsItem *d_items, const KsItem *d_sources, int B, int U, const KsItem *d_groups, int G,
                      int ell, hipStream_t s, bool addend = false);
bool chain_fusion_supported(); // the continuation kernels exist for the default launch sequences only
// grouped-digit hybrid key switching (hybrid_ks.hip; Context::hybrid()): b_rotate_hops / b_mul_relin / keyswitch route here
void hyb_rotate_hops(Context &c, const BatchWs &w, const KsItem *d_items, int B, int ell, hipStream_t s, int unique = 0);
// lazy sums (option hyb_lazy_sum): the B items' accumulators are added group by group and divided by P once per group.  d_groups[g]: dst = the
// sum's destination, elt = first item of the group, slot = its item count (a group's items are adjacent in d_items; their own dst is unused)
void hyb_rotate_sum(Context &c, const BatchWs &w, const KsItem *d_items, int B, const KsItem *d_groups, int G, int ell, hipStream_t s, int unique = 0);
bool hyb_lazy_sum_supported(const Context &c);
// one rotation hop by value (the one-instruction-at-a-time loop): src must not alias dst
void hyb_rotate_hop_single(Context &c, const Workspace &w, CtView dst, CtView src, u32 galois_elt, const u64 *galois_key, int ell, hipStream_t s);
void hyb_mul_relin(Context &c, const BatchWs &w, const MulItem *d_items, const u64 *relin_key, int B, int ell, hipStream_t s);
void hyb_keyswitch(Context &c, const Workspace &w, CtView out, const u64 *base0, const u64 *base1, const u64 *target, const u64 *key, int ell,
                   hipStream_t s);
// NTT-equivalents of one key switch at level ell: (l + 1)(l + 2) for SEAL's scheme, G (l + ksp) + 2 ksp + 2 l with grouped digits
inline int64_t ks_ntt_count(const Context &c, int ell)
{
    return c.hybrid() ? (int64_t)c.hyb_groups(ell) * (ell + c.ksp) + 2 * c.ksp + 2 * ell : (int64_t)(ell + 1) * (ell + 2);
}
// op: Neg / Mul (ct * plain) / Copy ; b_polys as in launch_ew
void b_ew(Context &c, EwOp op, const EwItem *d_items, int B, int polys, int b_polys, int ell, hipStream_t s);
void b_add_plain(Context &c, const EwItem *d_items, int B, int ell, hipStream_t s);
void b_sum(Context &c, const SumItem *d_items, const SumSrc *d_srcs, int B, int ell, hipStream_t s);
void b_sum_group(Context &c, const SumGroup *d_groups, const SumGroupSrc *d_gsrcs, int G, int ell, hipStream_t s);
// ModRaise (extension opcode 18): items[b].a at 1 prime -> items[b].dst at `target` primes, the centred residues mod q_0 re-read
// modulo every prime.  `scratch` holds [B][2][N]; h_items is the host copy of the items (the forward NTTs are launched per item).
void modraise(Context &c, u64 *scratch, const EwItem *h_items, int B, int target, hipStream_t s, const EwItem *d_items = nullptr);

// fused phase launchers (fused_ks.hip)
void f_irows_strided(const Context &c, const u64 *base, long stride, int prime_base, int period, u64 *out, long out_stride, int count,
                     hipStream_t s);
void f_irows_rot_c1(const Context &c, const KsItem *items, int ell, u64 *out, int B, hipStream_t s);
void f_irows_rs_last(const Context &c, const RsItem *items, const SumSrc *srcs, int l, u64 *out, int B, hipStream_t s);
void f_irows_rs_single(const Context &c, CtView src, int l, u64 *out, hipStream_t s);
void f_irows_decrypt(const Context &c, CtView ct, const u64 *sk, int ell, u64 *out, hipStream_t s);
// first inverse phase of a1*b1 of every item (the tensor product's c2, computed in the loader)
void f_irows_tensor_c2(const Context &c, const MulItem *items, int ell, u64 *out, int B, hipStream_t s);
// ... of sum_k s_k a_k1*b_k1 of every item (b_mul_sum_relin); the sum itself is also stored to target[B][ell][N] (NTT form), where the key
// switch's middle reads the digit a modulus owns
void f_irows_tensor_sum(const Context &c, const MulSumItem *items, const MulTerm *terms, int ell, u64 *out, u64 *target, int B, hipStream_t s);
// last forward phase of b_mul_sum_relin: dst = base + (acc - t) P^-1 with base = (sum_k s_k d_k0, sum_k s_k d_k1) computed in the epilogue
// (terms != nullptr; mode 4's term-walking form) or already lying in dst (terms == nullptr; mode 1's)
void f_frows_sum_final(const Context &c, const u64 *tmp, const MulSumItem *items, const MulTerm *terms, const u64 *acc, int B, int ell,
                       hipStream_t s);
// batched opcode 10: inverse ROWS phase of c0 + c1*s of every item -> out[B][ell][N] ...
void f_irows_decrypt_items(const Context &c, const BootItem *items, const SumSrc *srcs, const u64 *sk, int ell, u64 *out, int B,
                           hipStream_t s);
// the phases of b_mul_relin_rescale that differ from b_mul_relin's: first inverse phase of a1*b1 from a MulRsItem table; the fused middle
// whose row l - 1 leaves as an inverse ROWS phase with P (d + A) added; both divisions in one COLS launch; the last ROWS phase
void f_irows_tensor_c2_rs(const Context &c, const MulRsItem *items, int ell, u64 *out, int B, hipStream_t s);
void f_ks_frows_mac_rs(const Context &c, const u64 *ext, const MulRsItem *items, const u64 *relin_key, u64 *acc, int B, int ell, hipStream_t s);
void f_dr2_icols_lift_fcols(const Context &c, const u64 *acc, const MulRsItem *items, u64 *tmp, int B, int ell, hipStream_t s);
void f_frows_fold_final(const Context &c, const u64 *tmp, const MulRsItem *items, const u64 *acc, int B, int ell, hipStream_t s,
                        const Handoff &h = Handoff{});
// re-encode + reduce + first forward phase in one launch (ell == 1: every target limb recomputes the trivial composition):
// pt [B][ell][N] coefficient domain -> ptx [B][t][N] after the COLS phase
void f_boot_reencode_fcols(const Context &c, const u64 *pt, u64 *ptx, const BootItem *items, int B, int ell, int t, CrtDev crt,
                           hipStream_t s);
// ... and the last forward phase of the re-encoded plaintexts ptx[B][t][N], added to the items' zero-encryptions
void f_frows_boot_final(const Context &c, const u64 *ptx, const BootItem *items, int B, int t, hipStream_t s);
void f_ks_icols_lift_fcols(const Context &c, const u64 *digits, u64 *ext, int B, int ell, hipStream_t s);
void f_dr_icols_lift_fcols(const Context &c, const u64 *last, long last_stride, u64 *tmp, int polys, int cnt, int l, hipStream_t s);
// The divide-and-round of B zero-encryptions pk_p * NTT(u_b) + NTT(e_{b,p}) by prime l, from NTT(u) alone (fused_ks.hip, "zero-encryptions"):
// inverse ROWS phase of pk_{p,l} * NTT(u_b)_l -> out[B][2][N]; the middle kernel, which adds [e]_{q_l} after the inverse COLS phase and
// subtracts [e]_{q_i} from each lifted polynomial before its forward COLS phase (noise[B][2][N], one signed byte per coefficient); the
// last ROWS phase with pk_{p,i} * NTT(u_b)_i formed in its epilogue, written to the items' destinations.  pk: [2][K][N], NTT form.
void f_irows_zenc(const Context &c, const ZencItem *items, const u64 *pk, int l, u64 *out, int B, hipStream_t s);
void f_dr_noise_icols_lift_fcols(const Context &c, const u64 *last, long last_stride, u64 *tmp, int polys, int cnt, int l,
                                 const signed char *noise, hipStream_t s);
void f_frows_zenc_final(const Context &c, const u64 *tmp, const ZencItem *items, const u64 *pk, int B, int l, hipStream_t s);
// L3 + L4 + L5 fused (small batches): second NTT phase of the lifted digits, inner products with the key, first inverse phase of
// the special-prime accumulators.  mode 0 rotation (items[b].key, operand through the Galois permutation) / 1 relinearisation
// fold_base (rotations): the accumulators of the data primes leave with P galois(c0) added, and f_frows_final is told so (base_folded)
void f_ks_frows_mac(const Context &c, int mode, const u64 *ext, const u64 *target, const KsItem *items, const u64 *shared_key, u64 *acc,
                    int B, int ell, hipStream_t s, bool fold_base = false);
// large-batch variants: inverse COLS phase run separately (once per source limb), then base change + forward COLS
void f_ks_lift_fcols(const Context &c, const u64 *digits, u64 *ext, int B, int ell, hipStream_t s);
void f_dr_lift_fcols(const Context &c, const u64 *last, long last_stride, u64 *tmp, int polys, int cnt, int l, hipStream_t s);
// mode 0 rotation / 1 relinearisation / 2 rescale items / 3 one rescale by value (+ optional plaintext added to c0) /
// 4 relinearisation with the c0, c1 tensor terms computed in the epilogue (small batches: no tensor launch)
void f_frows_final(const Context &c, int mode, const u64 *tmp, const void *items, const u64 *acc, int polys, int cnt, int l,
                   hipStream_t s, RsItem single = RsItem{}, const u64 *plain = nullptr, const SumSrc *srcs = nullptr,
                   const Handoff &h = Handoff{}, bool base_folded = false);
// out[i][k] = residues[i] for i < ell: a constant polynomial's limbs in NTT form (batch_ops.hip)
void fill_const_plain(Context &c, u64 *out, const u64 *d_residues, int ell, hipStream_t s);
// a single rescale_to_next of `src` (level ell) into dst, optionally adding a level-(ell-1) plaintext to c0: 3 launches
void rescale_fused(Context &c, const Workspace &w, CtView dst, CtView src, int ell, const u64 *plain, hipStream_t s);

} // namespace dacapo
