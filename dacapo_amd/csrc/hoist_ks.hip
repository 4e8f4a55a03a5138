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
#include "ntt_tile.hpp"
#include "plan.hpp"
#include "tile_dispatch.hpp"

namespace dacapo {

typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// GaloisTool::apply_galois_ntt index map (fused_ks.hip galois_idx)
__device__ __forceinline__ u32 hoist_galois_idx(u32 k, u32 elt, int logN)
{
    const u32 r = (__brev(k) >> (32 - logN)) * 2u + 1u;
    const u32 idx = ((elt * r) >> 1) & ((1u << logN) - 1u);
    return __brev(idx) >> (32 - logN);
}

// grid = (tiles, l + 2 - MERGE, B) or, items_fast, (tiles, B, l + 2 - MERGE): the rows and item order of f_ks_frows_mac_kernel.  Workgroup
// (tile, y, b) owns the tile's coefficients of output modulus slot m (y < l: prime y, both accumulators; above: the special prime) of hop b:
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
    static_assert(E >= 2, "pairs");
    const int y = items_fast ? blockIdx.z : blockIdx.y, b = items_fast ? blockIdx.y : blockIdx.z, sp = Kp - 1;
    const int m = y < ell ? y : ell, psel = (MERGE && y == ell) ? -1 : y - ell; // psel < 0: both accumulators
    const int pm = m == ell ? sp : m;
    const size_t N = (size_t)1 << logN;
    const DModulus M = mods[pm];
    const KsItem it = items[b];
    const int g0 = tile_gidx<K, LOGE, false>(NP - 1, logN, blockIdx.x, 0);
    u32 gi[E / 2];
#pragma unroll
    for (int h = 0; h < E / 2; h++) gi[h] = hoist_galois_idx((u32)(g0 + 2 * h), it.elt, logN);
    auto gather = [&](u64(&x)[E], const u64 *__restrict__ p) {
#pragma unroll
        for (int h = 0; h < E / 2; h++) {
            const u64x2 v = *reinterpret_cast<const u64x2 *>(p + (gi[h] & ~1u));
            x[2 * h] = (gi[h] & 1u) ? v.y : v.x, x[2 * h + 1] = (gi[h] & 1u) ? v.x : v.y;
        }
    };
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
        if ((j & 15) == 15 && j + 1 < ell) { // a 128-bit accumulator holds 16 products of canonical residues (Acc128): fold it into a word
#pragma unroll
            for (int e = 0; e < E; e++) {
                const u64 f0 = a0[e].reduce(M), f1 = a1[e].reduce(M);
                a0[e].clear(), a1[e].clear();
                a0[e].lo = f0, a1[e].lo = f1;
            }
        }
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

// geometry and merging as f_ks_frows_mac chooses them (options tiny_tile_wgs, ks_merge_special_min_wgs, ks_items_fast)
static void f_ks_gmac(const Context &c, const u64 *L, const KsItem *items, u64 *acc, int B, int ell, hipStream_t s)
{
#define DC_GMAC(LEV)                                                                                                                      \
    {                                                                                                                                     \
        constexpr int LE = LEV;                                                                                                           \
        const long wgs = (long)(c.N >> TileGeo<LE>::LOG) * (ell + 2) * B;                                                                \
        const int merge = wgs >= (long)option(OPT_KS_MERGE_SPECIAL_MIN_WGS) ? 1 : 0;                                                      \
        const int items_fast = (B > 1 && B <= 65535 && option(OPT_KS_ITEMS_FAST)) ? 1 : 0;                                               \
        const dim3 grid((unsigned)(c.N >> TileGeo<LE>::LOG), (unsigned)(items_fast ? B : ell + 2 - merge), (unsigned)(items_fast ? ell + 2 - merge : B)); \
        if (merge) {                                                                                                                      \
            DC_K_SWITCH(c.k2, DC_LAUNCH((f_ks_gmac_kernel<KK, LE, true>), grid, dim3(kTileThreads), 0, s, L, items, acc, ell, c.K, c.d_mods, \
                                        c.d_itw, c.logN, c.d_pmod, items_fast));                                                          \
        } else {                                                                                                                          \
            DC_K_SWITCH(c.k2, DC_LAUNCH((f_ks_gmac_kernel<KK, LE, false>), grid, dim3(kTileThreads), 0, s, L, items, acc, ell, c.K, c.d_mods, \
                                        c.d_itw, c.logN, c.d_pmod, items_fast));                                                          \
        }                                                                                                                                 \
    }
    if (use_tiny_tiles(c.N, (long)(ell + 2) * B))
        DC_GMAC(1)
    else
        DC_GMAC(2)
#undef DC_GMAC
}

// B hops over U decompositions.  d_items[b].slot names the hop's source among d_sources[0 .. U) (items with the identity element whose
// src is the source ciphertext).  Scratch: w.digits [U][l][N], w.ext [U][l*l][N] (the decompositions), w.acc [B][2][l+1][N], w.tmp [B][2][l][N]
// -- U <= B, so a BatchWs sized for B default hops holds it.  A hop's destination may be its source: every read of a source precedes the
// last launch, the only one that writes a destination.
void hoist_rotate_hops(Context &c, const BatchWs &w, const KsItem *d_items, const KsItem *d_sources, int B, int U, int ell, hipStream_t s)
{
    if (c.hybrid()) {
        fprintf(stderr, "[dacapo_amd] hoisted rotations are for SEAL-layout keys: grouped-digit key switching (ks_special > 1) already shares "
                        "the decomposition among the hops of a source\n");
        abort();
    }
    if (B < 1 || U < 1 || U > B || ell < 1 || ell > c.max_level()) {
        fprintf(stderr, "[dacapo_amd] hoist_rotate_hops: %d hops over %d sources at level %d\n", B, U, ell);
        abort();
    }
    const size_t N = c.N;
    const int sp = c.K - 1;
    const long big = (long)option(OPT_KS_BIG_TILES);
    // decompose: U x l digits, each lifted to its l other moduli, stored in NTT form
    f_irows_rot_c1(c, d_sources, ell, w.digits, U, s);
    if ((long)(N >> 10) * U * ell * ell >= big) {
        launch_ntt_cols_inv(c, w.digits, (long)N, U * ell, nullptr, 0, ell, s);
        f_ks_lift_fcols(c, w.digits, w.ext, U, ell, s);
    } else
        f_ks_icols_lift_fcols(c, w.digits, w.ext, U, ell, s);
    launch_ntt_rows_fwd(c, w.ext, (long)N, U * ell * ell, c.ks_prime_idx(ell), 0, ell * ell, s);
    // per hop: inner products through the Galois map, then the default sequence's mod-down
    f_ks_gmac(c, w.ext, d_items, w.acc, B, ell, s);
    u64 *acc_last = w.acc + (size_t)ell * N;
    const long acc_ps = (long)(ell + 1) * (long)N;
    if ((long)(N >> 10) * B * ell * ell >= big) {
        launch_ntt_cols_inv(c, acc_last, acc_ps, 2 * B, nullptr, sp, 1, s);
        f_dr_lift_fcols(c, acc_last, acc_ps, w.tmp, 2 * B, ell, sp, s);
    } else
        f_dr_icols_lift_fcols(c, acc_last, acc_ps, w.tmp, 2 * B, ell, sp, s);
    f_frows_final(c, 0, w.tmp, d_items, w.acc, 2 * B, ell, sp, s, RsItem{}, nullptr, nullptr, Handoff{}, true);
}

} // namespace dacapo
