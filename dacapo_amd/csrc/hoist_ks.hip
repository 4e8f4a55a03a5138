// Hoisted rotations on SEAL-layout keys (option ks_hoist, dc_ct_rotate_hoisted): the hops of ONE source ciphertext share its decomposition.
//
// A rotation hop of the default sequence (fused_ks.hip) permutes c1 first and then decomposes it: inverse NTT, every digit lifted to every
// other modulus, forward NTT of the l*l lifted limbs -- per HOP.  That decomposition of the un-permuted c1 depends on the source alone, and
// a ring automorphism maps a valid decomposition of c1 to a valid decomposition of galois(c1).  So here the digits are taken BEFORE the
// automorphism, once per source, stored complete in NTT form
//     L[u][j][e][N]    u = source, j = digit, e = the e-th other modulus of digit j (ks_other_prime: the data primes but j, then the special one)
// (the layout of BatchWs::ext; the diagonal L[j][j] is c1's own limb j and is read in place, never copied), and every hop reads them through
// its Galois permutation in the NTT domain.  r hops of one source at level l transform l(l + 1) limbs instead of r l(l + 1).
//
// Not SEAL's rounding: a negated coefficient's non-centred lift differs by q_i mod q_j, so every limb differs from the default hop's -- by a
// multiple of Q in the message part and ordinary switching noise otherwise.  The definition is oracle/ckks_oracle.c orc_rotate_ks_hybrid at
// one special prime and one prime per digit, limb for limb, whether or not anything is shared.
//
// Launches of a batch of B hops over U sources:
//   f_irows_rot_c1 (identity element)  ->  [icols] + lift + fcols (fused_ks.hip, U items)  ->  launch_ntt_rows_fwd over the U l*l limbs (stores)
//   f_ks_gmac (B items: gather + inner products + base term + first inverse phase of the special prime)
//   [icols] -> f_dr_(icols_)lift_fcols -> f_frows_final        the default sequence's tail, unchanged
//
// Lazy sums (option ks_lazy_sum, dc_ct_rotate_sum_hoisted): G sums  dst_g = sum_k [pt_k] galois_k(src_k)  of B members over U sources divide by P
// ONCE per sum.  The decomposition stage is the same; f_ks_gsum takes the place of f_ks_gmac -- a workgroup walks the members of its group and
// leaves ONE accumulator pair per group -- and the tail runs over 2G polynomials instead of 2B.  The definition is the oracle's
// orc_rotate_acc_hybrid per member, Oracle.lazy_mul_plain / lazy_add, and one orc_moddown_hybrid per group, limb for limb.
//
// Shared with f_ks_frows_mac_kernel (ks_mac.hpp, galois.hpp): the row decode ks_row, the fold ks_fold, the Galois pair indices and gather, and the
// host's launch-shape rule ks_mac_shape / ks_mac_dispatch.  The digit step and the finish are written out in both kernels below, on purpose:
// as shared functions they cost registers (ks_mac.hpp, profiles/ks_mac_regs.txt).
#include "ks_mac.hpp"

namespace dacapo {

// grid = (tiles, l + 2 - MERGE, B) or, items_fast, (tiles, B, l + 2 - MERGE): the rows and item order of f_ks_frows_mac_kernel (ks_mac.hpp ks_row).
// Workgroup (tile, y, b) owns the tile's coefficients of output modulus slot m (y < l: prime y, both accumulators; above: the special prime) of hop b:
//   acc_c[m] = sum_j L[slot][j][m][pi(.)] key[j][c][m][.]   (+ P c0[m][pi(.)] on acc_0 of a data prime: the base term, as in the fused middle)
// A thread holds 2^LOGE CONSECUTIVE coefficients (the last-pass layout of a ROWS tile, which the special prime's inverse phase starts from):
// the map sends an aligned pair of outputs to an aligned pair of inputs, possibly swapped, so every gather is 16-byte loads, and the pair
// indices are computed once for all the digits.  The gather is the only uncoalesced access; keys and accumulators move as 16-byte vectors.
// No transform runs in the digit loop: the LDS tile is touched by the special prime's inverse phase only.
template <int K, int LOGE, bool MERGE>
__global__ __launch_bounds__(kTileThreads) void f_ks_gmac_kernel(const u64 *__restrict__ L, const KsItem *__restrict__ items, u64 *__restrict__ acc,
                                                                  int ell, int Kp, const DModulus *__restrict__ mods, const u64 *__restrict__ itw,
                                                                  int logN, const u64 *__restrict__ pmod, int items_fast)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    constexpr int E = 1 << LOGE, NP = num_passes<LOGE>(K);
    const KsRow r = ks_row<MERGE>(blockIdx, ell, Kp, items_fast);
    const int b = r.b, m = r.m, psel = r.psel, pm = r.pm, sp = Kp - 1;
    const size_t N = (size_t)1 << logN;
    const DModulus M = mods[pm];
    const KsItem it = items[b];
    const int g0 = tile_gidx<K, LOGE, false>(NP - 1, logN, blockIdx.x, 0);
    u32 gi[E / 2];
    galois_pair_idx<E>(gi, (u32)g0, it.elt, logN);
    auto gather = [&](u64(&x)[E], const u64 *__restrict__ p) { galois_gather<E>(x, p, gi); };
    Acc128 a0[E], a1[E];
#pragma unroll
    for (int e = 0; e < E; e++) a0[e].clear(), a1[e].clear();
    if (m < ell) { // the accumulator's start value, below 2^60 like a folded window (f_ks_frows_mac_kernel)
        u64 cv[E];
        gather(cv, it.src.limb(0, m, N));
        const u64 P = pmod[m];
#pragma unroll
        for (int e = 0; e < E; e++) a0[e].lo = mulmod(cv[e], P, M);
    }
    const u64 *Ls = L + (size_t)it.slot * ell * ell * N;
    for (int j = 0; j < ell; j++) {
        const u64 *src = j == m ? it.src.limb(1, j, N) : Ls + ((size_t)j * ell + (m < j ? m : m - 1)) * N;
        const u64 *k0 = it.key + (((size_t)j * 2 + 0) * Kp + pm) * N + g0, *k1 = it.key + (((size_t)j * 2 + 1) * Kp + pm) * N + g0;
        u64 x[E];
        gather(x, src);
        if (psel != 1) {
#pragma unroll
            for (int h = 0; h < E / 2; h++) {
                const u64x2 kv = *reinterpret_cast<const u64x2 *>(k0 + 2 * h);
                a0[2 * h].mac(x[2 * h], kv.x), a0[2 * h + 1].mac(x[2 * h + 1], kv.y);
            }
        }
        if (psel != 0) {
#pragma unroll
            for (int h = 0; h < E / 2; h++) {
                const u64x2 kv = *reinterpret_cast<const u64x2 *>(k1 + 2 * h);
                a1[2 * h].mac(x[2 * h], kv.x), a1[2 * h + 1].mac(x[2 * h + 1], kv.y);
            }
        }
        if ((j & 15) == 15 && j + 1 < ell) ks_fold<E>(a0, a1, M);
    }
    if (m < ell) {
        u64 *ac = acc + (size_t)b * 2 * (ell + 1) * N;
        u64 *o0 = ac + ((size_t)0 * (ell + 1) + m) * N + g0, *o1 = ac + ((size_t)1 * (ell + 1) + m) * N + g0;
#pragma unroll
        for (int h = 0; h < E / 2; h++) {
            u64x2 r0, r1;
            r0.x = a0[2 * h].reduce(M), r0.y = a0[2 * h + 1].reduce(M), r1.x = a1[2 * h].reduce(M), r1.y = a1[2 * h + 1].reduce(M);
            *reinterpret_cast<u64x2 *>(o0 + 2 * h) = r0, *reinterpret_cast<u64x2 *>(o1 + 2 * h) = r1;
        }
    } else { // the special prime's accumulators continue in registers into the inverse ROWS phase the mod-down starts with
        auto nold = [](int) -> u64 { return 0; };
        const int p_lo = MERGE ? 0 : psel, p_hi = MERGE ? 1 : psel;
        for (int p = p_lo; p <= p_hi; p++) {
            u64 r[E];
#pragma unroll
            for (int e = 0; e < E; e++) r[e] = p == 0 ? a0[e].reduce(M) : a1[e].reduce(M);
            u64 *o = acc + (((size_t)b * 2 + p) * (ell + 1) + ell) * N;
            if (p != p_lo) __syncthreads(); // the previous tile's last LDS image has been read by everyone
            ntt_tile_x<K, LOGE, false, true, false, true, false>(r, M, itw + ((size_t)sp << logN), logN, blockIdx.x, nold,
                                                                 [=](int gidx, u64 v) { o[gidx] = v; }, lds);
        }
    }
}

// geometry and merging as f_ks_frows_mac chooses them (ks_mac.hpp ks_mac_shape)
static void f_ks_gmac(const Context &c, const u64 *L, const KsItem *items, u64 *acc, int B, int ell, hipStream_t s)
{
    const KsMacShape sh = ks_mac_shape(c, ell, B);
    ks_mac_dispatch(c.k2, sh, [&](auto k, auto le, auto merge) {
        DC_LAUNCH((f_ks_gmac_kernel<decltype(k)::value, decltype(le)::value, decltype(merge)::value>), sh.grid, dim3(kTileThreads), 0, s, L, items,
                  acc, ell, c.K, c.d_mods, c.d_itw, c.logN, c.d_pmod, sh.items_fast);
    });
}

// The group form of f_ks_gmac_kernel: grid = (tiles, l + 2 - MERGE, G) or, groups_fast, (tiles, G, l + 2 - MERGE).  Workgroup (tile, y, g) owns the
// tile's coefficients of output modulus slot m of GROUP g (groups[g]: dst, elt = first member in items, slot = member count) and walks the
// members: per member the pair indices once, the digits gathered through the member's own permutation from the member's own source's
// decomposition (items[k].slot), the inner products with the member's key, and the base term P galois_k(c0_k) on acc_0 of a data prime -- here
// one more PRODUCT (c0 . P) instead of a reduced start value, because a member may join accumulators that are already in use.
//   bare member:        its products go straight into the group's accumulators s0, s1;
//   plaintext member:   they go into accumulators a0, a1 of its own, which are reduced to canonical words and multiplied by the plaintext's
//                       limb at m (plain [level][N] on a data prime, plain_sp [1][N] on the special one): one more mac per accumulator.
// An Acc128 holds 16 products of canonical residues.  What has landed in an accumulator since its last fold is COUNTED (ns for the group's pair,
// na for a member's; wave-uniform) and the pair is folded to canonical words -- which then count as one product -- before a 17th would join:
// 63 members x l digits pass through one pair.  Every stored limb is canonical and modular sums are exact in any order, so the result does not
// depend on where the folds fall.  The finish is f_ks_gmac_kernel's.
// ADDEND (dc_ct_rotate_sum_hoisted_add; option ks_flatten_sums): groups[g].src is a ciphertext at the group's level that is added to the sum
// exactly (p == nullptr: this group has none) -- one more product P . addend_p on accumulator p of every data prime, counted like any other,
// and nothing on the special prime: a multiple of P changes neither the rounding term nor the quotient's remainder, so every limb is
// Oracle.add(addend, the sum without it).  The addend is read where it lies (no permutation), before any member; only the last launch of
// the sequence writes a destination, so it may be a source or the destination.  A flag, so that the forms without it compile as before.
template <int K, int LOGE, bool MERGE, bool ADDEND = false>
__global__ __launch_bounds__(kTileThreads) void f_ks_gsum_kernel(const u64 *__restrict__ L, const KsItem *__restrict__ items,
                                                                  const KsItem *__restrict__ groups, u64 *__restrict__ acc, int ell, int Kp,
                                                                  const DModulus *__restrict__ mods, const u64 *__restrict__ itw, int logN,
                                                                  const u64 *__restrict__ pmod, int groups_fast)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    constexpr int E = 1 << LOGE, NP = num_passes<LOGE>(K);
    const KsRow r = ks_row<MERGE>(blockIdx, ell, Kp, groups_fast);
    const int g = r.b, m = r.m, psel = r.psel, pm = r.pm, sp = Kp - 1;
    const size_t N = (size_t)1 << logN;
    const DModulus M = mods[pm];
    const KsItem gr = groups[g];
    const KsItem *mem = items + gr.elt;
    const int cnt = (int)gr.slot;
    const int g0 = tile_gidx<K, LOGE, false>(NP - 1, logN, blockIdx.x, 0);
    const u64 P = m < ell ? pmod[m] : 0;
    auto room = [&](Acc128(&x0)[E], Acc128(&x1)[E], int &n) { // one more product per accumulator is about to land
        if (n == 16) ks_fold<E>(x0, x1, M), n = 1;
        n++;
    };
    Acc128 s0[E], s1[E];
#pragma unroll
    for (int e = 0; e < E; e++) s0[e].clear(), s1[e].clear();
    int ns = 0;
    if constexpr (ADDEND) {
        if (m < ell && gr.src.p) {
            const u64 *d0 = gr.src.limb(0, m, N) + g0, *d1 = gr.src.limb(1, m, N) + g0;
            room(s0, s1, ns);
#pragma unroll
            for (int h = 0; h < E / 2; h++) {
                const u64x2 v0 = *reinterpret_cast<const u64x2 *>(d0 + 2 * h), v1 = *reinterpret_cast<const u64x2 *>(d1 + 2 * h);
                s0[2 * h].mac(v0.x, P), s0[2 * h + 1].mac(v0.y, P), s1[2 * h].mac(v1.x, P), s1[2 * h + 1].mac(v1.y, P);
            }
        }
    }
    for (int k = 0; k < cnt; k++) {
        const KsItem it = mem[k];
        u32 gi[E / 2];
        galois_pair_idx<E>(gi, (u32)g0, it.elt, logN);
        auto gather = [&](u64(&x)[E], const u64 *__restrict__ p) { galois_gather<E>(x, p, gi); };
        const u64 *Ls = L + (size_t)it.slot * ell * ell * N;
        auto products = [&](Acc128(&x0)[E], Acc128(&x1)[E], int &n) { // the member's base term and inner products into (x0, x1)
            if (m < ell) {
                u64 cv[E];
                gather(cv, it.src.limb(0, m, N));
                room(x0, x1, n);
#pragma unroll
                for (int e = 0; e < E; e++) x0[e].mac(cv[e], P);
            }
            for (int j = 0; j < ell; j++) {
                const u64 *src = j == m ? it.src.limb(1, j, N) : Ls + ((size_t)j * ell + (m < j ? m : m - 1)) * N;
                const u64 *k0 = it.key + (((size_t)j * 2 + 0) * Kp + pm) * N + g0, *k1 = it.key + (((size_t)j * 2 + 1) * Kp + pm) * N + g0;
                u64 x[E];
                gather(x, src);
                room(x0, x1, n);
                if (psel != 1) {
#pragma unroll
                    for (int h = 0; h < E / 2; h++) {
                        const u64x2 kv = *reinterpret_cast<const u64x2 *>(k0 + 2 * h);
                        x0[2 * h].mac(x[2 * h], kv.x), x0[2 * h + 1].mac(x[2 * h + 1], kv.y);
                    }
                }
                if (psel != 0) {
#pragma unroll
                    for (int h = 0; h < E / 2; h++) {
                        const u64x2 kv = *reinterpret_cast<const u64x2 *>(k1 + 2 * h);
                        x1[2 * h].mac(x[2 * h], kv.x), x1[2 * h + 1].mac(x[2 * h + 1], kv.y);
                    }
                }
            }
        };
        if (!it.plain) {
            products(s0, s1, ns);
            continue;
        }
        Acc128 a0[E], a1[E];
#pragma unroll
        for (int e = 0; e < E; e++) a0[e].clear(), a1[e].clear();
        int na = 0;
        products(a0, a1, na);
        const u64 *pt = (m < ell ? it.plain + (size_t)m * N : it.plain_sp) + g0;
        room(s0, s1, ns);
#pragma unroll
        for (int h = 0; h < E / 2; h++) {
            const u64x2 w = *reinterpret_cast<const u64x2 *>(pt + 2 * h);
            if (psel != 1) s0[2 * h].mac(a0[2 * h].reduce(M), w.x), s0[2 * h + 1].mac(a0[2 * h + 1].reduce(M), w.y);
            if (psel != 0) s1[2 * h].mac(a1[2 * h].reduce(M), w.x), s1[2 * h + 1].mac(a1[2 * h + 1].reduce(M), w.y);
        }
    }
    if (m < ell) {
        u64 *ac = acc + (size_t)g * 2 * (ell + 1) * N;
        u64 *o0 = ac + ((size_t)0 * (ell + 1) + m) * N + g0, *o1 = ac + ((size_t)1 * (ell + 1) + m) * N + g0;
#pragma unroll
        for (int h = 0; h < E / 2; h++) {
            u64x2 r0, r1;
            r0.x = s0[2 * h].reduce(M), r0.y = s0[2 * h + 1].reduce(M), r1.x = s1[2 * h].reduce(M), r1.y = s1[2 * h + 1].reduce(M);
            *reinterpret_cast<u64x2 *>(o0 + 2 * h) = r0, *reinterpret_cast<u64x2 *>(o1 + 2 * h) = r1;
        }
    } else { // the special prime's accumulators continue in registers into the inverse ROWS phase the mod-down starts with
        auto nold = [](int) -> u64 { return 0; };
        const int p_lo = MERGE ? 0 : psel, p_hi = MERGE ? 1 : psel;
        for (int p = p_lo; p <= p_hi; p++) {
            u64 r[E];
#pragma unroll
            for (int e = 0; e < E; e++) r[e] = p == 0 ? s0[e].reduce(M) : s1[e].reduce(M);
            u64 *o = acc + (((size_t)g * 2 + p) * (ell + 1) + ell) * N;
            if (p != p_lo) __syncthreads(); // the previous tile's last LDS image has been read by everyone
            ntt_tile_x<K, LOGE, false, true, false, true, false>(r, M, itw + ((size_t)sp << logN), logN, blockIdx.x, nold,
                                                                 [=](int gidx, u64 v) { o[gidx] = v; }, lds);
        }
    }
}

// geometry and merging chosen as f_ks_gmac chooses them, with groups in the place of hops; addend: the groups' src fields are addends (or null)
static void f_ks_gsum(const Context &c, const u64 *L, const KsItem *items, const KsItem *groups, u64 *acc, int G, int ell, bool addend, hipStream_t s)
{
    const KsMacShape sh = ks_mac_shape(c, ell, G);
    ks_mac_dispatch(c.k2, sh, [&](auto k, auto le, auto merge) {
        if (addend)
            DC_LAUNCH((f_ks_gsum_kernel<decltype(k)::value, decltype(le)::value, decltype(merge)::value, true>), sh.grid, dim3(kTileThreads), 0, s, L,
                      items, groups, acc, ell, c.K, c.d_mods, c.d_itw, c.logN, c.d_pmod, sh.items_fast);
        else
            DC_LAUNCH((f_ks_gsum_kernel<decltype(k)::value, decltype(le)::value, decltype(merge)::value>), sh.grid, dim3(kTileThreads), 0, s, L, items,
                      groups, acc, ell, c.K, c.d_mods, c.d_itw, c.logN, c.d_pmod, sh.items_fast);
    });
}

// B hops over U decompositions.  d_items[b].slot names the hop's source among d_sources[0 .. U) (items with the identity element whose
// src is the source ciphertext).  Scratch: w.digits [U][l][N], w.ext [U][l*l][N] (the decompositions), w.acc [B][2][l+1][N], w.tmp [B][2][l][N]
// -- U <= B, so a BatchWs sized for B default hops holds it.  A hop's destination may be its source: every read of a source precedes the
// last launch, the only one that writes a destination.
static void hoist_check(const Context &c, const char *who, int B, int U, int G, int ell)
{
    if (c.hybrid()) {
        fprintf(stderr, "[dacapo_amd] hoisted rotations are for SEAL-layout keys: grouped-digit key switching (ks_special > 1) already shares "
                        "the decomposition among the hops of a source\n");
        abort();
    }
    if (B < 1 || U < 1 || U > B || G < 1 || G > B || ell < 1 || ell > c.max_level()) {
        fprintf(stderr, "[dacapo_amd] %s: %d hops over %d sources in %d sums at level %d\n", who, B, U, G, ell);
        abort();
    }
}

// decompose: U x l digits, each lifted to its l other moduli, stored in NTT form in w.ext
static void hoist_decompose(Context &c, const BatchWs &w, const KsItem *d_sources, int U, int ell, hipStream_t s)
{
    const size_t N = c.N;
    f_irows_rot_c1(c, d_sources, ell, w.digits, U, s);
    if ((long)(N >> 10) * U * ell * ell >= (long)option(OPT_KS_BIG_TILES)) {
        launch_ntt_cols_inv(c, w.digits, (long)N, U * ell, nullptr, 0, ell, s);
        f_ks_lift_fcols(c, w.digits, w.ext, U, ell, s);
    } else
        f_ks_icols_lift_fcols(c, w.digits, w.ext, U, ell, s);
    launch_ntt_rows_fwd(c, w.ext, (long)N, U * ell * ell, c.ks_prime_idx(ell), 0, ell * ell, s);
}

// the default sequence's mod-down over R accumulator pairs w.acc [R][2][l+1][N] (the special prime's limbs after their first inverse phase, the
// base terms folded in); d_dsts[r].dst is where pair r goes
static void hoist_moddown(Context &c, const BatchWs &w, const KsItem *d_dsts, int R, int ell, hipStream_t s)
{
    const size_t N = c.N;
    const int sp = c.K - 1;
    u64 *acc_last = w.acc + (size_t)ell * N;
    const long acc_ps = (long)(ell + 1) * (long)N;
    if ((long)(N >> 10) * R * ell * ell >= (long)option(OPT_KS_BIG_TILES)) {
        launch_ntt_cols_inv(c, acc_last, acc_ps, 2 * R, nullptr, sp, 1, s);
        f_dr_lift_fcols(c, acc_last, acc_ps, w.tmp, 2 * R, ell, sp, s);
    } else
        f_dr_icols_lift_fcols(c, acc_last, acc_ps, w.tmp, 2 * R, ell, sp, s);
    f_frows_final(c, 0, w.tmp, d_dsts, w.acc, 2 * R, ell, sp, s, RsItem{}, nullptr, nullptr, Handoff{}, true);
}

void hoist_rotate_hops(Context &c, const BatchWs &w, const KsItem *d_items, const KsItem *d_sources, int B, int U, int ell, hipStream_t s)
{
    hoist_check(c, "hoist_rotate_hops", B, U, 1, ell);
    hoist_decompose(c, w, d_sources, U, ell, s);
    // per hop: inner products through the Galois map, then the default sequence's mod-down
    f_ks_gmac(c, w.ext, d_items, w.acc, B, ell, s);
    hoist_moddown(c, w, d_items, B, ell, s);
}

// G lazy sums of B members over U decompositions: d_groups[g] = { dst: the sum's destination, elt: its first member in d_items, slot: its
// member count } (a group's members are adjacent; their own dst is unused), d_items[b].slot / d_sources as above, d_items[b].plain / plain_sp the
// plaintext multiplying member b in the raised basis, or null.  Scratch: w.digits / w.ext as above, w.acc [G][2][l+1][N], w.tmp [G][2][l][N]
// -- U, G <= B.  A destination may be one of the sources: only the last launch writes, and it reads no source.
// addend: d_groups[g].src is a ciphertext added to sum g exactly (src.p == nullptr: none), read by the inner-product launch alone -- it may be
// a source or a destination of the batch; false: the field is not read.
void hoist_rotate_sum(Context &c, const BatchWs &w, const KsItem *d_items, const KsItem *d_sources, int B, int U, const KsItem *d_groups, int G,
                      int ell, hipStream_t s, bool addend)
{
    hoist_check(c, "hoist_rotate_sum", B, U, G, ell);
    hoist_decompose(c, w, d_sources, U, ell, s);
    f_ks_gsum(c, w.ext, d_items, d_groups, w.acc, G, ell, addend, s);
    hoist_moddown(c, w, d_groups, G, ell, s);
}

} // namespace dacapo
