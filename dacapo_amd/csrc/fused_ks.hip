// Fused phase kernels of the batched key-switch / rescale pipelines (plan.hpp, batch_ops.hip).
//
// A key switch at level l is  iNTT(l limbs) -> lift each digit to the l other moduli -> NTT(l*l limbs) -> inner
// products with the key -> mod-down (iNTT of the special-prime limb, lift, NTT, scale) [SEAL-upstream
// Evaluator::switch_key_inplace, reached from SEAL_HEVM.cpp:273,316].  Launched phase by phase that is 13 dependent
// launches; at the HEVM working levels (2-5 primes) each is microseconds of work, so the launch chain IS the latency.
// The tile routine lets an inverse COLS phase hand its canonical output to a forward COLS phase in registers, so:
//   L1 irows   : inverse ROWS phase, reading the operand in place (Galois gather fused into the loader)
//   L2 icols+lift+fcols : per (digit j, other modulus e): finish the iNTT of digit j, reduce into q_e, first NTT phase
//   L3 frows   : second NTT phase over the l*l lifted digits
//   L4 mac     : inner products with the key (the j == m term reads the operand in place)
//   L5 irows   : special-prime limb of both accumulators
//   L6 icols+round+fcols : finish its iNTT, add floor(P/2), reduce into q_i, subtract, first NTT phase
//   L7 frows+final : second NTT phase, (acc - t) * P^-1 + base, written straight into the destination
// 7 launches instead of 13; rescale is L5'-L7' = 3 instead of 7.  (Round 3: throughput-bound launches take MERGE instantiations of L2 / L6
// / L3-L5 that do not repeat work per target modulus / per accumulator; see the kernels.)  L2/L6 recompute the inverse COLS phase once per
// target modulus (it is 1/(l+1) of that kernel's work) to keep every workgroup at two phases.
#include "ks_mac.hpp"

namespace dacapo {

// ---- operand sources of the first inverse phase ----------------------------------------------------------------------
struct SrcStrided { // limb z at base + z*stride, modulo prime prime_base + z % period
    const u64 *base;
    long stride;
    int prime_base, period;
    __device__ int prime(int z) const { return prime_base + z % period; }
    __device__ u64 load(int z, int g, int) const { return base[(long)z * stride + g]; }
};
// Operand of a rescale item (plan.hpp RsItem) for the E coefficients a thread owns: elementwise producers (n-ary sum,
// + plaintext, * plaintext) that nothing else reads are evaluated here instead of being materialised.  Modular
// arithmetic is exact, so the values equal what the separate ops would have stored.  Every stage issues its E loads
// together (term loop outermost) -- a per-coefficient evaluation would serialise one memory latency per term.
template <int E>
__device__ __forceinline__ void rs_operand(u64 (&v)[E], const int (&g)[E], const RsItem &it, const SumSrc *__restrict__ srcs, int p, int i,
                                           size_t N, const DModulus &M)
{
    if (it.count == 0) {
        const u64 *x = it.src.limb(p, i, N);
#pragma unroll
        for (int j = 0; j < E; j++) v[j] = x[g[j]];
    } else {
        u64 s[E];
        Acc128 a[E];
#pragma unroll
        for (int j = 0; j < E; j++) s[j] = 0, a[j].clear();
        int n_plain = 0, n_prod = 0;
        for (int t = 0; t < it.count; t++) {
            const SumSrc src = srcs[it.first + t];
            const u64 *x = src.v.limb(p, i, N);
            if (src.plain) {
                const u64 *w = src.plain + (size_t)i * N;
#pragma unroll
                for (int j = 0; j < E; j++) a[j].mac(x[g[j]], w[g[j]]);
                if ((++n_prod & 15) == 0) {
#pragma unroll
                    for (int j = 0; j < E; j++) s[j] = fold60(s[j], M.delta) + a[j].reduce(M), a[j].clear();
                }
            } else {
#pragma unroll
                for (int j = 0; j < E; j++) s[j] += x[g[j]];
                if ((++n_plain & 7) == 0) {
#pragma unroll
                    for (int j = 0; j < E; j++) s[j] = fold60(s[j], M.delta);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < E; j++) v[j] = addmod(canon(s[j], M), a[j].reduce(M), M.q);
    }
    if (it.add && p == 0) {
        const u64 *w = it.add + (size_t)i * N;
#pragma unroll
        for (int j = 0; j < E; j++) v[j] = addmod(v[j], w[g[j]], M.q);
    }
    if (it.mul) {
        const u64 *w = it.mul + (size_t)i * N;
#pragma unroll
        for (int j = 0; j < E; j++) v[j] = mulmod(v[j], w[g[j]], M);
    }
}

// opcode 10, first launch: Decryptor::decrypt (c0 + c1*s) of every item's operand fused into the first inverse phase.
// z = b*ell + i.  The operand may be an expression (a rescale folded into the opcode, with what had been folded into it).
template <int K, int LOGE>
__global__ __launch_bounds__(kTileThreads) void f_irows_boot_kernel(const BootItem *__restrict__ items, const SumSrc *__restrict__ srcs,
                                                                     const u64 *__restrict__ sk, int ell, u64 *__restrict__ out,
                                                                     const DModulus *__restrict__ mods, const u64 *__restrict__ itw,
                                                                     int logN)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    constexpr int E = 1 << LOGE;
    const int z = blockIdx.y, i = z % ell;
    const size_t N = (size_t)1 << logN;
    const BootItem bi = items[z / ell];
    const RsItem it{ bi.src, bi.dst, bi.first, bi.count, bi.add, bi.mul };
    const DModulus M = mods[i];
    const u64 *s = sk + (size_t)i * N;
    u64 *o = out + (size_t)z * N;
    int g[E];
#pragma unroll
    for (int j = 0; j < E; j++) g[j] = tile_gidx<K, LOGE, false>(num_passes<LOGE>(K) - 1, logN, blockIdx.x, j);
    u64 x[E], x1[E];
    rs_operand<E>(x, g, it, srcs, 0, i, N, M);
    rs_operand<E>(x1, g, it, srcs, 1, i, N, M);
#pragma unroll
    for (int j = 0; j < E; j++) x[j] = addmod(x[j], mulmod(x1[j], s[g[j]], M), M.q);
    auto nold = [](int) -> u64 { return 0; };
    ntt_tile_x<K, LOGE, false, true, false, true, false>(x, M, itw + ((size_t)i << logN), logN, blockIdx.x, nold,
                                                         [=](int gi, u64 v) { o[gi] = v; }, lds);
}

// R1: inverse ROWS phase of the limb a rescale drops.  z = b*2 + p
template <int K, int LOGE>
__global__ __launch_bounds__(kTileThreads) void f_irows_rs_kernel(const RsItem *__restrict__ items, const SumSrc *__restrict__ srcs, int l,
                                                                   u64 *__restrict__ out, const DModulus *__restrict__ mods,
                                                                   const u64 *__restrict__ itw, int logN)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    constexpr int E = 1 << LOGE;
    const int z = blockIdx.y;
    const size_t N = (size_t)1 << logN;
    const DModulus M = mods[l];
    u64 *o = out + (size_t)z * N;
    int g[E];
#pragma unroll
    for (int j = 0; j < E; j++) g[j] = tile_gidx<K, LOGE, false>(num_passes<LOGE>(K) - 1, logN, blockIdx.x, j);
    u64 x[E];
    rs_operand<E>(x, g, items[z >> 1], srcs, z & 1, l, N, M);
    auto nold = [](int) -> u64 { return 0; };
    ntt_tile_x<K, LOGE, false, true, false, true, false>(x, M, itw + ((size_t)l << logN), logN, blockIdx.x, nold,
                                                         [=](int gi, u64 v) { o[gi] = v; }, lds);
}

struct SrcRsLast1 { // single rescale without a device item table (encryption's divide-and-round)
    CtView src;
    int l;
    __device__ int prime(int) const { return l; }
    __device__ u64 load(int z, int g, int logN) const { return src.limb(z & 1, l, (size_t)1 << logN)[g]; }
};
struct SrcDecrypt { // limb z of c0 + c1*s  (Decryptor::decrypt fused into the first inverse phase)
    CtView ct;
    const u64 *sk;
    const DModulus *mods;
    __device__ int prime(int z) const { return z; }
    __device__ u64 load(int z, int g, int logN) const
    {
        const size_t N = (size_t)1 << logN;
        const DModulus M = mods[z];
        return addmod(ct.limb(0, z, N)[g], mulmod(ct.limb(1, z, N)[g], sk[(size_t)z * N + g], M), M.q);
    }
};

template <class Item> // MulItem, or MulRsItem (a multiply with its rescale folded in)
struct SrcTensorC2 { // limb z = b*ell + i of a1*b1, the c2 of item b's tensor product (ckks_multiply) -- never materialised
    const Item *items;
    const DModulus *mods;
    int ell;
    __device__ int prime(int z) const { return z % ell; }
    __device__ u64 load(int z, int g, int logN) const
    {
        const size_t N = (size_t)1 << logN;
        const int i = z % ell;
        const Item &it = items[z / ell];
        return mulmod(it.a.limb(1, i, N)[g], it.b.limb(1, i, N)[g], mods[i]);
    }
};
// L1 / L5 / R1: inverse ROWS phase, out[z] (lazy values) = phase(src limb z)
template <int K, int LOGE, class Src>
__global__ __launch_bounds__(kTileThreads) void f_irows_kernel(Src src, u64 *__restrict__ out, long out_stride,
                                                                const DModulus *__restrict__ mods, const u64 *__restrict__ itw,
                                                                int logN)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    const int z = blockIdx.y, p = src.prime(z);
    u64 *o = out + (long)z * out_stride;
    ntt_tile<K, LOGE, false, true, false>(
        mods[p], itw + ((size_t)p << logN), logN, blockIdx.x, [=](int g) { return src.load(z, g, logN); },
        [=](int g, u64 v) { o[g] = v; }, lds);
}

// ---- sums of signed ct x ct products relinearised once (plan.hpp MulSumItem, b_mul_sum_relin) ----------------------------------------------
// Component COMP of sum_k s_k (a_k (x) b_k) at limb i, for the E coefficients g[] a thread owns: 0 = a0 b0, 1 = a0 b1 + a1 b0, 2 = a1 b1.
// Terms of either sign gather in an accumulator of their own and the canonical difference is taken once at the end: modular arithmetic is
// exact, so the value is what tensor + poly_add / poly_sub give term by term, in any order.
// Ranges (modarith.hpp): an operand is a canonical residue, at most q - 1 < 2^60, so a product is below 2^120 and Acc128 takes 16 of them with
// hi < 2^60, the precondition of reduce128_lazy.  A term adds at most 2 products (COMP 1) to ONE accumulator; both are folded every 8 terms
// -- at most 16 products since the last fold -- and a folded accumulator restarts from its canonical residue, one more term below 2^60:
// 16 (q - 1)^2 + 2^60 < 2^124 for operands q - 1 throughout, whatever the count and the signs.
template <int E, int COMP>
__device__ __forceinline__ void tensor_sum(u64 (&v)[E], const int (&g)[E], const MulTerm *__restrict__ terms, int first, int count, int i, size_t N,
                                           const DModulus &M)
{
    Acc128 pos[E], neg[E];
#pragma unroll
    for (int j = 0; j < E; j++) pos[j].clear(), neg[j].clear();
    auto mac_all = [&](Acc128(&a)[E], const u64 *x, const u64 *y) {
#pragma unroll
        for (int j = 0; j < E; j++) a[j].mac(x[g[j]], y[g[j]]);
    };
    for (int t = 0; t < count; t++) {
        const MulTerm tm = terms[first + t];
        const u64 *x = tm.a.limb(COMP == 2 ? 1 : 0, i, N), *y = tm.b.limb(COMP == 0 ? 0 : 1, i, N);
        if (tm.sign > 0) // (wave-uniform)
            mac_all(pos, x, y);
        else
            mac_all(neg, x, y);
        if (COMP == 1) {
            const u64 *x1 = tm.a.limb(1, i, N), *y0 = tm.b.limb(0, i, N);
            if (tm.sign > 0)
                mac_all(pos, x1, y0);
            else
                mac_all(neg, x1, y0);
        }
        if ((t & 7) == 7 && t + 1 < count) {
#pragma unroll
            for (int j = 0; j < E; j++) {
                const u64 fp = pos[j].reduce(M), fn = neg[j].reduce(M);
                pos[j].clear(), neg[j].clear();
                pos[j].lo = fp, neg[j].lo = fn;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < E; j++) v[j] = submod(pos[j].reduce(M), neg[j].reduce(M), M.q);
}

// L1 of a product sum: the term-walking form of f_irows_kernel<SrcTensorC2>.  z = b*ell + i.  The sum's c2 limb also goes to target[z] in NTT
// form: the key switch's middle reads the digit a modulus owns from there (f_ks_frows_mac_kernel with a target, as it stands).
template <int K, int LOGE>
__global__ __launch_bounds__(kTileThreads) void f_irows_tensor_sum_kernel(const MulSumItem *__restrict__ items, const MulTerm *__restrict__ terms,
                                                                           int ell, u64 *__restrict__ out, u64 *__restrict__ target,
                                                                           const DModulus *__restrict__ mods, const u64 *__restrict__ itw, int logN)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    constexpr int E = 1 << LOGE;
    const int z = blockIdx.y, i = z % ell;
    const size_t N = (size_t)1 << logN;
    const MulSumItem it = items[z / ell];
    const DModulus M = mods[i];
    u64 *o = out + (size_t)z * N, *tg = target + (size_t)z * N;
    int g[E];
#pragma unroll
    for (int j = 0; j < E; j++) g[j] = tile_gidx<K, LOGE, false>(num_passes<LOGE>(K) - 1, logN, blockIdx.x, j);
    u64 x[E];
    tensor_sum<E, 2>(x, g, terms, it.first, it.count, i, N, M);
#pragma unroll
    for (int j = 0; j < E; j++) tg[g[j]] = x[j];
    auto nold = [](int) -> u64 { return 0; };
    ntt_tile_x<K, LOGE, false, true, false, true, false>(x, M, itw + ((size_t)i << logN), logN, blockIdx.x, nold,
                                                         [=](int gi, u64 v) { o[gi] = v; }, lds);
}

// L7 of a product sum: the term-walking form of f_frows_final_kernel mode 4 (TENSOR: the base terms sum_k s_k d_k0 / sum_k s_k d_k1 are
// computed in the epilogue; dst holds nothing yet and must not be an operand) and of mode 1 (!TENSOR: a tensor-sum launch left them in dst).
// z = (b*2 + p)*cnt + i
template <int K, int LOGE, bool TENSOR>
__global__ __launch_bounds__(kTileThreads) void f_frows_sum_final_kernel(const u64 *__restrict__ tmp, const MulSumItem *__restrict__ items,
                                                                          const MulTerm *__restrict__ terms, const u64 *__restrict__ acc, int cnt,
                                                                          int l, int Kp, const DModulus *__restrict__ mods,
                                                                          const u64 *__restrict__ inv_last, const u64 *__restrict__ tw, int logN)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    constexpr int E = 1 << LOGE;
    const int z = blockIdx.y, i = z % cnt, bp = z / cnt, b = bp >> 1, p = bp & 1;
    const size_t N = (size_t)1 << logN;
    const DModulus M = mods[i];
    const u64 inv = inv_last[(size_t)l * Kp + i];
    const u64 *in = tmp + (size_t)z * N;
    const MulSumItem it = items[b];
    const u64 *x = acc + (((size_t)bp) * (cnt + 1) + i) * N;
    u64 *o = it.dst.limb(p, i, N);
    u64 v[E], base[E];
    int g[E];
    auto nost = [](int, u64) {};
    ntt_tile_x<K, LOGE, false, false, true, false, true>(v, M, tw + ((size_t)i << logN), logN, blockIdx.x, [=](int gi) { return in[gi]; }, nost, lds);
#pragma unroll
    for (int j = 0; j < E; j++) g[j] = tile_gidx<K, LOGE, false>(num_passes<LOGE>(K) - 1, logN, blockIdx.x, j);
    if (!TENSOR) {
#pragma unroll
        for (int j = 0; j < E; j++) base[j] = o[g[j]];
    } else if (p == 0)
        tensor_sum<E, 0>(base, g, terms, it.first, it.count, i, N, M);
    else
        tensor_sum<E, 1>(base, g, terms, it.first, it.count, i, N, M);
#pragma unroll
    for (int j = 0; j < E; j++) o[g[j]] = addmod(base[j], mulmod(submod(x[g[j]], v[j], M.q), inv, M), M.q);
}

// ---- L2 / L6 / R2: inverse COLS phase, base change, first forward phase -------------------------------------------------------------------
// (Their target loop is written out in f_ks_, f_dr_ and f_dr2_icols_lift_fcols_kernel: as one function with a per-target functor every
// listing changes, f_ks_icols_lift_fcols_kernel<7, 2, true> 89 -> 90 VGPRs; profiles/fused_tail_share.txt)

// L2: z = (b*l + j)*l + e
// MERGE (throughput-bound launches, grid.y = B*l): one workgroup finishes the iNTT of digit (b, j) ONCE and runs the base change + first
// NTT phase for each of its l target moduli in turn, instead of l workgroups each recomputing the inverse phase (a quarter of the
// launch's work at l = 2, a third at l = 3) -- what the large-batch path gets from two launches and a round trip through HBM.
template <int K, int LOGE, bool MERGE>
__global__ __launch_bounds__(kTileThreads) void f_ks_icols_lift_fcols_kernel(const u64 *__restrict__ digits, u64 *__restrict__ ext,
                                                                              int ell, int sp, const DModulus *__restrict__ mods,
                                                                              const u64 *__restrict__ tw, const u64 *__restrict__ itw,
                                                                              int logN, const u64 *__restrict__ tw2)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    const int z = blockIdx.y, dj = MERGE ? z : z / ell, j = dj % ell;
    const size_t N = (size_t)1 << logN;
    const u64 *in = digits + (size_t)dj * N;
    u64 x[1 << LOGE];
    auto nost = [](int, u64) {};
    ntt_tile_x<K, LOGE, true, true, true, false, true>(
        x, mods[j], itw + ((size_t)j << logN), logN, blockIdx.x, [=](int g) { return in[g]; }, nost, lds);
    auto nold = [](int) -> u64 { return 0; };
    for (int e = MERGE ? 0 : z % ell; e < (MERGE ? ell : z % ell + 1); e++) {
        u64 *out = ext + ((size_t)dj * ell + e) * N;
        const int pm = ks_other_prime(j, e, ell, sp);
        const DModulus Mm = mods[pm];
        u64 y[1 << LOGE];
#pragma unroll
        for (int r = 0; r < (1 << LOGE); r++) y[r] = recanon(x[r], Mm); // one conditional subtraction within a width class (modarith.hpp)
        __syncthreads(); // the previous tile's last LDS image has been read by everyone
        ntt_tile_fcols<K, LOGE, false, true, false>(
            y, Mm, tw + ((size_t)pm << logN), tw2 ? tw2 + ((size_t)pm << (K + 1)) : nullptr, logN, blockIdx.x, nold, [=](int g, u64 v) { out[g] = v; }, lds);
    }
}

// RNSTool::divide_and_round_q_last_ntt_inplace, coefficient-domain part: rho = x + floor(q_l / 2) mod q_l ...
__device__ __forceinline__ u64 dr_round(u64 x, u64 half, u64 ql)
{
    const u64 y = x + half;
    return y >= ql ? y - ql : y;
}
// ... reduced into q_i, - floor(q_l / 2) mod q_i  (neg_half = q_i - (floor(q_l / 2) mod q_i))
__device__ __forceinline__ u64 dr_reduce(u64 rho, const DModulus &Mi, u64 neg_half)
{
    const u64 v = recanon(rho, Mi) + neg_half;
    return v >= Mi.q ? v - Mi.q : v;
}

// L6 / R2: z = bp*cnt + i : finish the iNTT of the dropped limb bp (prime l), round, change base to prime i, first NTT phase
// MERGE (grid.y = polys): the same sharing as in L2 -- the dropped limb's inverse phase once, then every target modulus in turn
// NOISE: the middle kernel of a zero-encryption (f_irows_zenc_kernel below); `noise` is null otherwise.  An inverse COLS tile ends with
// pass 0: register r holds coefficient tile_gidx<K, LOGE, true>(0, ..., r), which is where this thread's bytes of e are.
template <int K, int LOGE, bool MERGE, bool NOISE>
__global__ __launch_bounds__(kTileThreads) void f_dr_icols_lift_fcols_kernel(const u64 *__restrict__ last, long last_stride,
                                                                              u64 *__restrict__ tmp, int cnt, int l, int Kp,
                                                                              const DModulus *__restrict__ mods,
                                                                              const u64 *__restrict__ half_mod,
                                                                              const u64 *__restrict__ tw, const u64 *__restrict__ itw,
                                                                              int logN, const u64 *__restrict__ tw2,
                                                                              const signed char *__restrict__ noise)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    const int z = blockIdx.y, bp = MERGE ? z : z / cnt;
    const size_t N = (size_t)1 << logN;
    const u64 *in = last + (long)bp * last_stride;
    u64 x[1 << LOGE];
    int e[1 << LOGE];
    if (NOISE) {
        const signed char *ep = noise + (size_t)bp * N;
#pragma unroll
        for (int r = 0; r < (1 << LOGE); r++) e[r] = ep[tile_gidx<K, LOGE, true>(0, logN, blockIdx.x, r)];
    }
    auto nost = [](int, u64) {};
    ntt_tile_x<K, LOGE, true, true, true, false, true>(
        x, mods[l], itw + ((size_t)l << logN), logN, blockIdx.x, [=](int g) { return in[g]; }, nost, lds);
    const u64 ql = mods[l].q, half = ql >> 1;
#pragma unroll
    for (int r = 0; r < (1 << LOGE); r++) { // (+ [e]_{q_l},) then + floor(q_l / 2), both mod q_l
        if (NOISE) {
            const u64 y = x[r] + (e[r] < 0 ? ql - (u64)(-e[r]) : (u64)e[r]);
            x[r] = y >= ql ? y - ql : y;
        }
        x[r] = dr_round(x[r], half, ql);
    }
    auto nold = [](int) -> u64 { return 0; };
    for (int i = MERGE ? 0 : z % cnt; i < (MERGE ? cnt : z % cnt + 1); i++) {
        u64 *out = tmp + ((size_t)bp * cnt + i) * N;
        const DModulus Mi = mods[i];
        const u64 qi = Mi.q, neg_half = qi - half_mod[(size_t)l * Kp + i];
        u64 y[1 << LOGE];
#pragma unroll
        for (int r = 0; r < (1 << LOGE); r++) { // (NOISE: - [e]_{q_i})
            u64 v = dr_reduce(x[r], Mi, neg_half);
            if (NOISE) {
                v += e[r] > 0 ? qi - (u64)e[r] : (u64)(-e[r]);
                v = v >= qi ? v - qi : v;
            }
            y[r] = v;
        }
        __syncthreads(); // the previous tile's last LDS image has been read by everyone
        ntt_tile_fcols<K, LOGE, false, true, false>(
            y, Mi, tw + ((size_t)i << logN), tw2 ? tw2 + ((size_t)i << (K + 1)) : nullptr, logN, blockIdx.x, nold, [=](int g, u64 v) { out[g] = v; }, lds);
    }
}

// ---- zero-encryptions of a plan (HEVM::plan_zero_encrypt, option zenc_head = 1) -----------------------------------------------------------
// rescale(pk_p * U + NTT(e_p)) over the primes 0..l, U = NTT(u), from U alone: the three kernels of a rescale (R1 - R3 above) with the
// key's product formed in the first and the last one and the noise e_p -- small signed coefficients, one byte each, never transformed --
// joining in the coefficient domain of the middle one:
//   delta = iNTT_l(pk_{p,l} * U_l) + [e_p]_{q_l}     rho = [delta + floor(q_l/2)]_{q_l}     t_i = (rho mod q_i) - (floor(q_l/2) mod q_i)
//   z_i   = q_l^-1 (pk_{p,i} * U_i - NTT_i(t_i - [e_p]_{q_i}))  =  q_l^-1 ((pk_{p,i} * U_i + NTT_i(e_p)) - NTT_i(t_i))      exactly, mod q_i
// A ROWS tile's first inverse / last forward pass gives a thread 2^LOGE CONSECUTIVE coefficients: the loaders and the epilogue run on
// 16-byte vectors.  z = b*2 + p in the first two kernels, (b*2 + p)*l + i in the last.
template <int K, int LOGE>
__global__ __launch_bounds__(kTileThreads) void f_irows_zenc_kernel(const ZencItem *__restrict__ items, const u64 *__restrict__ pk, long pk_ps,
                                                                     int l, u64 *__restrict__ out, const DModulus *__restrict__ mods,
                                                                     const u64 *__restrict__ itw, int logN)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    constexpr int E = 1 << LOGE;
    const int z = blockIdx.y;
    const size_t N = (size_t)1 << logN;
    const DModulus M = mods[l];
    u64 *o = out + (size_t)z * N;
    const int g0 = tile_gidx<K, LOGE, false>(num_passes<LOGE>(K) - 1, logN, blockIdx.x, 0);
    const u64 *u = items[z >> 1].u + (size_t)l * N + g0, *k = pk + (z & 1) * pk_ps + (size_t)l * N + g0;
    u64 x[E];
#pragma unroll
    for (int j = 0; j < E; j += 2) {
        const u64x2 a = *reinterpret_cast<const u64x2 *>(u + j), b = *reinterpret_cast<const u64x2 *>(k + j);
        x[j] = mulmod(a.x, b.x, M), x[j + 1] = mulmod(a.y, b.y, M);
    }
    auto nold = [](int) -> u64 { return 0; };
    ntt_tile_x<K, LOGE, false, true, false, true, false>(x, M, itw + ((size_t)l << logN), logN, blockIdx.x, nold,
                                                         [=](int gi, u64 v) { o[gi] = v; }, lds);
}

// (the middle kernel is f_dr_icols_lift_fcols_kernel<K, LOGE, MERGE, NOISE = true>)
template <int K, int LOGE>
__global__ __launch_bounds__(kTileThreads) void f_frows_zenc_final_kernel(const u64 *__restrict__ tmp, const ZencItem *__restrict__ items,
                                                                           const u64 *__restrict__ pk, long pk_ps, int l, int Kp,
                                                                           const DModulus *__restrict__ mods,
                                                                           const u64 *__restrict__ inv_last, const u64 *__restrict__ tw,
                                                                           int logN)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    constexpr int E = 1 << LOGE;
    const int z = blockIdx.y, i = z % l, bp = z / l, b = bp >> 1, p = bp & 1;
    const size_t N = (size_t)1 << logN;
    const DModulus M = mods[i];
    const u64 inv = inv_last[(size_t)l * Kp + i];
    const u64 *in = tmp + (size_t)z * N;
    const ZencItem it = items[b];
    const int g0 = tile_gidx<K, LOGE, false>(num_passes<LOGE>(K) - 1, logN, blockIdx.x, 0);
    const u64 *u = it.u + (size_t)i * N + g0, *k = pk + p * pk_ps + (size_t)i * N + g0;
    u64 *o = it.dst.limb(p, i, N) + g0;
    u64 v[E];
    auto nost = [](int, u64) {};
    ntt_tile_x<K, LOGE, false, false, true, false, true>(v, M, tw + ((size_t)i << logN), logN, blockIdx.x, [=](int gi) { return in[gi]; }, nost, lds);
#pragma unroll
    for (int j = 0; j < E; j += 2) {
        const u64x2 a = *reinterpret_cast<const u64x2 *>(u + j), c = *reinterpret_cast<const u64x2 *>(k + j);
        u64x2 r;
        r.x = mulmod(submod(mulmod(a.x, c.x, M), v[j], M.q), inv, M), r.y = mulmod(submod(mulmod(a.y, c.y, M), v[j + 1], M.q), inv, M);
        *reinterpret_cast<u64x2 *>(o + j) = r;
    }
}

// L6 + R2 of a multiply whose rescale is folded in (option ks_fold_rescale): z = bp*cnt + i, cnt = l - 1 kept limbs.  Both dropped limbs of
// accumulator bp -- the special prime's (slot l of acc) and row l - 1's, which carries P (d + A) (f_ks_frows_mac_kernel, FOLD) -- finish their
// inverse transforms here, and per coefficient
//   rho = [X_P + floor(P/2)]_P                     t_i = (rho mod q_i) - (floor(P/2) mod q_i)
//   c   = s_L P^-1 (row_L - t_L)  mod q_L          u   = [c + floor(q_L/2)]_{q_L},  u_i = (u mod q_i) - (floor(q_L/2) mod q_i)
//   v_i = (s_i P^-1 t_i + u_i) q_L^-1              (L = l - 1; s the constant polynomial folded into the rescale, 1 when absent)
// is ONE lifted polynomial per kept limb, whose first NTT phase follows: SEAL's two roundings, limb for limb, from l - 1 forward
// transforms instead of 2l - 1.  Every step is exact arithmetic mod q_i.  MERGE as in f_dr_icols_lift_fcols_kernel.
// (the roundings are written out, not dr_round / dr_reduce: through the functions all 24 listings change, at the parent's VGPR counts; not timed)
template <int K, int LOGE, bool MERGE>
__global__ __launch_bounds__(kTileThreads) void f_dr2_icols_lift_fcols_kernel(const u64 *__restrict__ acc, const MulRsItem *__restrict__ items,
                                                                               u64 *__restrict__ tmp, int ell, int Kp,
                                                                               const DModulus *__restrict__ mods,
                                                                               const u64 *__restrict__ half_mod,
                                                                               const u64 *__restrict__ inv_last, const u64 *__restrict__ tw,
                                                                               const u64 *__restrict__ itw, int logN, const u64 *__restrict__ tw2)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    constexpr int E = 1 << LOGE;
    const int cnt = ell - 1, L = ell - 1, sp = Kp - 1;
    const int z = blockIdx.y, bp = MERGE ? z : z / cnt;
    const size_t N = (size_t)1 << logN;
    const u64 *in_p = acc + ((size_t)bp * (ell + 1) + ell) * N, *in_l = acc + ((size_t)bp * (ell + 1) + L) * N;
    const u64 *mul = items[bp >> 1].mul;
    const long mul_stride = items[bp >> 1].mul_stride;
    auto nost = [](int, u64) {};
    u64 rho[E], u[E];
    ntt_tile_x<K, LOGE, true, true, true, false, true>(
        rho, mods[sp], itw + ((size_t)sp << logN), logN, blockIdx.x, [=](int g) { return in_p[g]; }, nost, lds);
    __syncthreads(); // the tile's last LDS image has been read by everyone
    const DModulus ML = mods[L];
    ntt_tile_x<K, LOGE, true, true, true, false, true>(
        u, ML, itw + ((size_t)L << logN), logN, blockIdx.x, [=](int g) { return in_l[g]; }, nost, lds);
    {
        const u64 P = mods[sp].q, half_p = P >> 1, qL = ML.q, half_l = qL >> 1;
        const u64 neg_half = qL - half_mod[(size_t)sp * Kp + L];
        u64 k = inv_last[(size_t)sp * Kp + L]; // s_L P^-1 mod q_L
        if (mul) k = mulmod(mul[(long)L * mul_stride], k, ML);
#pragma unroll
        for (int r = 0; r < E; r++) {
            const u64 y = rho[r] + half_p;
            rho[r] = y >= P ? y - P : y;
            const u64 t = recanon(rho[r], ML) + neg_half;
            const u64 c = mulmod(submod(u[r], t >= qL ? t - qL : t, qL), k, ML) + half_l;
            u[r] = c >= qL ? c - qL : c;
        }
    }
    auto nold = [](int) -> u64 { return 0; };
    for (int i = MERGE ? 0 : z % cnt; i < (MERGE ? cnt : z % cnt + 1); i++) {
        u64 *out = tmp + ((size_t)bp * cnt + i) * N;
        const DModulus Mi = mods[i];
        const u64 qi = Mi.q, neg_half_p = qi - half_mod[(size_t)sp * Kp + i], neg_half_l = qi - half_mod[(size_t)L * Kp + i];
        const u64 k2 = inv_last[(size_t)L * Kp + i]; // q_L^-1 and s_i P^-1 q_L^-1 mod q_i
        u64 k3 = mulmod(inv_last[(size_t)sp * Kp + i], k2, Mi);
        if (mul) k3 = mulmod(mul[(long)i * mul_stride], k3, Mi);
        u64 y[E];
#pragma unroll
        for (int r = 0; r < E; r++) {
            const u64 t = recanon(rho[r], Mi) + neg_half_p, w = recanon(u[r], Mi) + neg_half_l;
            Acc128 a;
            a.clear();
            a.mac(t >= qi ? t - qi : t, k3);
            a.mac(w >= qi ? w - qi : w, k2);
            y[r] = a.reduce(Mi);
        }
        __syncthreads();
        ntt_tile_fcols<K, LOGE, false, true, false>(
            y, Mi, tw + ((size_t)i << logN), tw2 ? tw2 + ((size_t)i << (K + 1)) : nullptr, logN, blockIdx.x, nold, [=](int g, u64 v) { out[g] = v; }, lds);
    }
}

// Throughput variants of L2 / L6 for large batches: the inverse COLS phase has already been run once per source limb
// (launch_ntt_cols_inv, canonical output), so each workgroup only does the base change and ONE forward phase instead of
// recomputing the inverse phase per target modulus.
template <int K, int LOGE>
__global__ __launch_bounds__(kTileThreads) void f_ks_lift_fcols_kernel(const u64 *__restrict__ digits, u64 *__restrict__ ext, int ell,
                                                                        int sp, const DModulus *__restrict__ mods,
                                                                        const u64 *__restrict__ tw, int logN, const u64 *__restrict__ tw2)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    const int z = blockIdx.y, e = z % ell, dj = z / ell, j = dj % ell;
    const size_t N = (size_t)1 << logN;
    const u64 *in = digits + (size_t)dj * N;
    u64 *out = ext + (size_t)z * N;
    const int pm = ks_other_prime(j, e, ell, sp);
    const DModulus Mm = mods[pm];
    u64 x[1 << LOGE];
    ntt_tile_fcols<K, LOGE, false, false, false>(
        x, Mm, tw + ((size_t)pm << logN), tw2 ? tw2 + ((size_t)pm << (K + 1)) : nullptr, logN, blockIdx.x,
        [=](int g) {
            return recanon(in[g], Mm);
        },
        [=](int g, u64 v) { out[g] = v; }, lds);
}

template <int K, int LOGE>
__global__ __launch_bounds__(kTileThreads) void f_dr_lift_fcols_kernel(const u64 *__restrict__ last, long last_stride,
                                                                        u64 *__restrict__ tmp, int cnt, int l, int Kp,
                                                                        const DModulus *__restrict__ mods,
                                                                        const u64 *__restrict__ half_mod, const u64 *__restrict__ tw,
                                                                        int logN, const u64 *__restrict__ tw2)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    const int z = blockIdx.y, i = z % cnt, bp = z / cnt;
    const size_t N = (size_t)1 << logN;
    const u64 *in = last + (long)bp * last_stride;
    u64 *out = tmp + (size_t)z * N;
    const DModulus Mi = mods[i];
    const u64 ql = mods[l].q, half = ql >> 1;
    const u64 neg_half = Mi.q - half_mod[(size_t)l * Kp + i];
    u64 x[1 << LOGE];
    ntt_tile_fcols<K, LOGE, false, false, false>(
        x, Mi, tw + ((size_t)i << logN), tw2 ? tw2 + ((size_t)i << (K + 1)) : nullptr, logN, blockIdx.x,
        [=](int g) { return dr_reduce(dr_round(in[g], half, ql), Mi, neg_half); },
        [=](int g, u64 v) { out[g] = v; }, lds);
}

// L7 / R3: z = bp*cnt + i.  MODE 0 rotation, 1 relinearisation, 2 rescale
template <int K, int LOGE, int MODE>
__global__ __launch_bounds__(kTileThreads) void f_frows_final_kernel(const u64 *__restrict__ tmp, const void *__restrict__ items_,
                                                                      RsItem single, const u64 *__restrict__ plain,
                                                                      const SumSrc *__restrict__ srcs,
                                                                      const u64 *__restrict__ acc, int cnt, int l, int Kp,
                                                                      const DModulus *__restrict__ mods,
                                                                      const u64 *__restrict__ inv_last, const u64 *__restrict__ tw,
                                                                      int logN, int base_folded)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    const int z = blockIdx.y, i = z % cnt, bp = z / cnt, b = bp >> 1, p = bp & 1;
    const size_t N = (size_t)1 << logN;
    const DModulus M = mods[i];
    const u64 inv = inv_last[(size_t)l * Kp + i];
    const u64 *in = tmp + (size_t)z * N;
    if (MODE == 0 && base_folded) {
        // The rotation's base term galois(c0) already rides on the accumulator (f_ks_frows_mac_kernel added P galois(c0) to it:
        // galois(c0) + (acc - t) P^-1 = ((acc + P galois(c0)) - t) P^-1 exactly), so this kernel has no gather: a ROWS tile leaves a thread
        // 2^LOGE CONSECUTIVE coefficients and the epilogue runs on 16-byte vectors.  (The per-coefficient store functor below -- 8-byte accesses
        // at a 2^LOGE-word lane stride, a Galois gather with 64 lanes in 64 cache lines -- is what hybrid_fused.hip's last kernel measured 2.5x
        // slower than this form.)
        constexpr int E = 1 << LOGE;
        const KsItem it = reinterpret_cast<const KsItem *>(items_)[b];
        const u64 *x = acc + (((size_t)bp) * (cnt + 1) + i) * N;
        u64 *o = it.dst.limb(p, i, N);
        u64 v[E];
        auto nost = [](int, u64) {};
        ntt_tile_x<K, LOGE, false, false, true, false, true>(v, M, tw + ((size_t)i << logN), logN, blockIdx.x, [=](int gi) { return in[gi]; }, nost, lds);
        const int g0 = tile_gidx<K, LOGE, false>(num_passes<LOGE>(K) - 1, logN, blockIdx.x, 0);
#pragma unroll
        for (int j = 0; j < E; j += 2) {
            const u64x2 a = *reinterpret_cast<const u64x2 *>(x + g0 + j);
            u64x2 r;
            r.x = mulmod(submod(a.x, v[j], M.q), inv, M), r.y = mulmod(submod(a.y, v[j + 1], M.q), inv, M);
            *reinterpret_cast<u64x2 *>(o + g0 + j) = r;
        }
    } else if (MODE == 0) {
        const KsItem it = reinterpret_cast<const KsItem *>(items_)[b];
        const u64 *x = acc + (((size_t)bp) * (cnt + 1) + i) * N;
        const u64 *c0 = it.src.limb(0, i, N);
        u64 *o = it.dst.limb(p, i, N);
        ntt_tile<K, LOGE, false, false, true>(
            M, tw + ((size_t)i << logN), logN, blockIdx.x, [=](int g) { return in[g]; },
            [=](int g, u64 v) {
                const u64 base = p == 0 ? c0[galois_idx((u32)g, it.elt, logN)] : 0;
                o[g] = addmod(base, mulmod(submod(x[g], v, M.q), inv, M), M.q);
            },
            lds);
    } else if (MODE == 1) {
        const MulItem it = reinterpret_cast<const MulItem *>(items_)[b];
        const u64 *x = acc + (((size_t)bp) * (cnt + 1) + i) * N;
        u64 *o = it.dst.limb(p, i, N);
        ntt_tile<K, LOGE, false, false, true>(
            M, tw + ((size_t)i << logN), logN, blockIdx.x, [=](int g) { return in[g]; },
            [=](int g, u64 v) { o[g] = addmod(o[g], mulmod(submod(x[g], v, M.q), inv, M), M.q); }, lds);
    } else if (MODE == 4) { // relinearisation whose c0, c1 tensor terms are computed here (dst holds nothing yet)
        const MulItem it = reinterpret_cast<const MulItem *>(items_)[b];
        const u64 *x = acc + (((size_t)bp) * (cnt + 1) + i) * N;
        const u64 *a0 = it.a.limb(0, i, N), *a1 = it.a.limb(1, i, N), *b0 = it.b.limb(0, i, N), *b1 = it.b.limb(1, i, N);
        u64 *o = it.dst.limb(p, i, N);
        constexpr int E = 1 << LOGE;
        u64 v[E], base[E];
        int g[E];
        auto nost = [](int, u64) {};
        ntt_tile_x<K, LOGE, false, false, true, false, true>(v, M, tw + ((size_t)i << logN), logN, blockIdx.x,
                                                             [=](int gi) { return in[gi]; }, nost, lds);
#pragma unroll
        for (int j = 0; j < E; j++) g[j] = tile_gidx<K, LOGE, false>(num_passes<LOGE>(K) - 1, logN, blockIdx.x, j);
        if (p == 0) {
#pragma unroll
            for (int j = 0; j < E; j++) base[j] = mulmod(a0[g[j]], b0[g[j]], M);
        } else {
#pragma unroll
            for (int j = 0; j < E; j++) {
                Acc128 t;
                t.clear();
                t.mac(a0[g[j]], b1[g[j]]);
                t.mac(a1[g[j]], b0[g[j]]);
                base[j] = t.reduce(M);
            }
        }
#pragma unroll
        for (int j = 0; j < E; j++) o[g[j]] = addmod(base[j], mulmod(submod(x[g[j]], v[j], M.q), inv, M), M.q);
    } else if (MODE == 3) { // one rescale given by value, optionally followed by "+ plaintext" on c0 (Encryptor::encrypt)
        const u64 *x = single.src.limb(p, i, N);
        u64 *o = single.dst.limb(p, i, N);
        const u64 *pl = (plain && p == 0) ? plain + (size_t)i * N : nullptr;
        ntt_tile<K, LOGE, false, false, true>(
            M, tw + ((size_t)i << logN), logN, blockIdx.x, [=](int g) { return in[g]; },
            [=](int g, u64 v) {
                const u64 r = mulmod(submod(x[g], v, M.q), inv, M);
                o[g] = pl ? addmod(r, pl[g], M.q) : r;
            },
            lds);
    } else {
        const RsItem it = reinterpret_cast<const RsItem *>(items_)[b];
        u64 *o = it.dst.limb(p, i, N);
        constexpr int E = 1 << LOGE;
        u64 x[E], op[E];
        int g[E];
        auto nost = [](int, u64) {};
        ntt_tile_x<K, LOGE, false, false, true, false, true>(x, M, tw + ((size_t)i << logN), logN, blockIdx.x,
                                                             [=](int gi) { return in[gi]; }, nost, lds);
#pragma unroll
        for (int j = 0; j < E; j++) g[j] = tile_gidx<K, LOGE, false>(num_passes<LOGE>(K) - 1, logN, blockIdx.x, j);
        rs_operand<E>(op, g, it, srcs, p, i, N, M);
#pragma unroll
        for (int j = 0; j < E; j++) o[g[j]] = mulmod(submod(op[j], x[j], M.q), inv, M);
    }
}

// ---- L7 / R3 with a continuation into the consumer's first phase (plan.hpp Handoff) ---------------------------------------------------
// (Bodies written out more than once below, each with the figure of its shared form; the rest is in profiles/fused_tail_share.txt:
//   tensor terms, staged: f_frows_final_kernel<K, L, 4> up to +18 VGPRs, f_frows_final_cont_kernel<K, L, 4, CONT_RS> +20 to +42
//   continuations as device functions: 6-8 of the 12 listings of each form need more VGPRs, up to +20
//   MODE 2 / 4 epilogues through final_value, final_value MODE 0 without base_folded: every listing changes, not timed)
// Output polynomial p, limb i of item b at this tile's coefficients g[] (pass NP-1 layout of a ROWS tile): computed exactly as
// f_frows_final_kernel does for the same MODE, stored to the item's destination, and left in v[] (canonical).
template <int K, int LOGE, int MODE>
__device__ __forceinline__ void final_value(u64 (&v)[1 << LOGE], const int (&g)[1 << LOGE], const u64 *__restrict__ in, const void *__restrict__ items_,
                                            const SumSrc *__restrict__ srcs, const u64 *__restrict__ acc, int b, int p, int i, int cnt,
                                            const DModulus &M, u64 inv, const u64 *__restrict__ tw, int logN, u64 *__restrict__ lds,
                                            bool base_folded = false)
{
    constexpr int E = 1 << LOGE;
    const size_t N = (size_t)1 << logN;
    auto nost = [](int, u64) {};
    u64 x[E];
    ntt_tile_x<K, LOGE, false, false, true, false, true>(x, M, tw + ((size_t)i << logN), logN, blockIdx.x, [=](int gi) { return in[gi]; }, nost, lds);
    if (MODE == 4) {
        const MulItem it = reinterpret_cast<const MulItem *>(items_)[b];
        const u64 *ac = acc + (((size_t)(b * 2 + p)) * (cnt + 1) + i) * N;
        const u64 *a0 = it.a.limb(0, i, N), *a1 = it.a.limb(1, i, N), *b0 = it.b.limb(0, i, N), *b1 = it.b.limb(1, i, N);
        u64 *o = it.dst.limb(p, i, N);
#pragma unroll
        for (int j = 0; j < E; j++) {
            u64 base;
            if (p == 0)
                base = mulmod(a0[g[j]], b0[g[j]], M);
            else {
                Acc128 t;
                t.clear();
                t.mac(a0[g[j]], b1[g[j]]);
                t.mac(a1[g[j]], b0[g[j]]);
                base = t.reduce(M);
            }
            v[j] = addmod(base, mulmod(submod(ac[g[j]], x[j], M.q), inv, M), M.q);
            o[g[j]] = v[j];
        }
    } else if (MODE == 0) {
        const KsItem it = reinterpret_cast<const KsItem *>(items_)[b];
        const u64 *ac = acc + (((size_t)(b * 2 + p)) * (cnt + 1) + i) * N;
        const u64 *c0 = it.src.limb(0, i, N);
        u64 *o = it.dst.limb(p, i, N);
#pragma unroll
        for (int j = 0; j < E; j++) {
            const u64 base = (p == 0 && !base_folded) ? c0[galois_idx((u32)g[j], it.elt, logN)] : 0; // (folded: the accumulator carries it)
            v[j] = addmod(base, mulmod(submod(ac[g[j]], x[j], M.q), inv, M), M.q);
            o[g[j]] = v[j];
        }
    } else { // MODE 2: rescale
        const RsItem it = reinterpret_cast<const RsItem *>(items_)[b];
        u64 *o = it.dst.limb(p, i, N);
        u64 op[E];
        rs_operand<E>(op, g, it, srcs, p, i, N, M);
#pragma unroll
        for (int j = 0; j < E; j++) {
            v[j] = mulmod(submod(op[j], x[j], M.q), inv, M);
            o[g[j]] = v[j];
        }
    }
}

// CONT_RS / CONT_MUL: grid = (tiles, 2B * cnt), z = (b*2 + p)*cnt + i as in f_frows_final_kernel; the workgroups that hold what the
// consumer's first phase reads carry on.  CONT_BOOT: grid = (tiles, B * cnt), z = b*cnt + i, both polynomials in one workgroup
// (the consumer decrypts: c0 + c1*s).
template <int K, int LOGE, int MODE, int CONT>
__global__ __launch_bounds__(kTileThreads) void f_frows_final_cont_kernel(const u64 *__restrict__ tmp, const void *__restrict__ items_,
                                                                           const SumSrc *__restrict__ srcs, const u64 *__restrict__ acc, int cnt,
                                                                           int l, int Kp, const DModulus *__restrict__ mods,
                                                                           const u64 *__restrict__ inv_last, const u64 *__restrict__ tw,
                                                                           const u64 *__restrict__ itw, int logN, Handoff h, int base_folded)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    constexpr int E = 1 << LOGE, NP = num_passes<LOGE>(K);
    const size_t N = (size_t)1 << logN;
    int g[E];
#pragma unroll
    for (int j = 0; j < E; j++) g[j] = tile_gidx<K, LOGE, false>(NP - 1, logN, blockIdx.x, j);
    auto nold = [](int) -> u64 { return 0; };
    if (CONT == CONT_BOOT) {
        const int z = blockIdx.y, i = z % cnt, b = z / cnt;
        const DModulus M = mods[i];
        const u64 inv = inv_last[(size_t)l * Kp + i];
        u64 v0[E], v1[E];
        final_value<K, LOGE, MODE>(v0, g, tmp + ((size_t)(b * 2 + 0) * cnt + i) * N, items_, srcs, acc, b, 0, i, cnt, M, inv, tw, logN, lds, base_folded != 0);
        __syncthreads(); // the tile's last LDS image has been read by everyone
        final_value<K, LOGE, MODE>(v1, g, tmp + ((size_t)(b * 2 + 1) * cnt + i) * N, items_, srcs, acc, b, 1, i, cnt, M, inv, tw, logN, lds, base_folded != 0);
        const u64 *sk = h.sk + (size_t)i * N;
#pragma unroll
        for (int j = 0; j < E; j++) v0[j] = addmod(v0[j], mulmod(v1[j], sk[g[j]], M), M.q);
        __syncthreads();
        u64 *o = h.out + (size_t)z * N;
        ntt_tile_x<K, LOGE, false, true, false, true, false>(v0, M, itw + ((size_t)i << logN), logN, blockIdx.x, nold, [=](int gi, u64 v) { o[gi] = v; }, lds);
    } else {
        const int z = blockIdx.y, i = z % cnt, bp = z / cnt, b = bp >> 1, p = bp & 1;
        const DModulus M = mods[i];
        const u64 inv = inv_last[(size_t)l * Kp + i];
        u64 v[E];
        final_value<K, LOGE, MODE>(v, g, tmp + (size_t)z * N, items_, srcs, acc, b, p, i, cnt, M, inv, tw, logN, lds, base_folded != 0);
        if (CONT == CONT_RS) {
            if (i != cnt - 1) return; // the consumer drops the last limb: only its workgroups continue (uniform per workgroup)
            const RsItem cit = h.rs_items[b]; // single-use "+ plaintext" / "* plaintext" folded into the consumer (rs_operand's order)
            if (cit.add && p == 0) {
                const u64 *w = cit.add + (size_t)i * N;
#pragma unroll
                for (int j = 0; j < E; j++) v[j] = addmod(v[j], w[g[j]], M.q);
            }
            if (cit.mul) {
                const u64 *w = cit.mul + (size_t)i * N;
#pragma unroll
                for (int j = 0; j < E; j++) v[j] = mulmod(v[j], w[g[j]], M);
            }
            __syncthreads();
            u64 *o = h.out + (size_t)bp * N;
            ntt_tile_x<K, LOGE, false, true, false, true, false>(v, M, itw + ((size_t)i << logN), logN, blockIdx.x, nold, [=](int gi, u64 y) { o[gi] = y; }, lds);
        } else { // CONT_MUL
            if (p != 1) return;
            const CtView other = h.other[b];
            if (other.p) {
                const u64 *o1 = other.limb(1, i, N);
#pragma unroll
                for (int j = 0; j < E; j++) v[j] = mulmod(v[j], o1[g[j]], M);
            } else {
#pragma unroll
                for (int j = 0; j < E; j++) v[j] = mulmod(v[j], v[j], M);
            }
            __syncthreads();
            u64 *o = h.out + ((size_t)b * cnt + i) * N;
            ntt_tile_x<K, LOGE, false, true, false, true, false>(v, M, itw + ((size_t)i << logN), logN, blockIdx.x, nold, [=](int gi, u64 y) { o[gi] = y; }, lds);
        }
    }
}

// L7 + R3 of a multiply whose rescale is folded in: output polynomial p, kept limb i of item b at this tile's coefficients g[],
//   r_i = s_i q_L^-1 (X_i P^-1 + d_i + A_i) - NTT_i(v_i)
// (X the key-switch inner product, d the tensor term computed here as mode 4 of f_frows_final_kernel does, A the plaintext added to c0, v what
// f_dr2_icols_lift_fcols_kernel left), stored to the item's destination at level l - 1 and left in v[] (canonical).
template <int K, int LOGE>
__device__ __forceinline__ void fold_final_value(u64 (&v)[1 << LOGE], const int (&g)[1 << LOGE], const u64 *__restrict__ in, const MulRsItem &it,
                                                 const u64 *__restrict__ acc, int b, int p, int i, int ell, int Kp, const DModulus &M,
                                                 const u64 *__restrict__ inv_last, const u64 *__restrict__ tw, int logN, u64 *__restrict__ lds)
{
    constexpr int E = 1 << LOGE;
    const size_t N = (size_t)1 << logN;
    auto nost = [](int, u64) {};
    u64 x[E];
    ntt_tile_x<K, LOGE, false, false, true, false, true>(x, M, tw + ((size_t)i << logN), logN, blockIdx.x, [=](int gi) { return in[gi]; }, nost, lds);
    const u64 pinv = inv_last[(size_t)(Kp - 1) * Kp + i];
    u64 k1 = inv_last[(size_t)(ell - 1) * Kp + i]; // s_i q_L^-1 mod q_i
    if (it.mul) k1 = mulmod(it.mul[(long)i * it.mul_stride], k1, M);
    const u64 *ac = acc + (((size_t)(b * 2 + p)) * (ell + 1) + i) * N;
    const u64 *a0 = it.a.limb(0, i, N), *a1 = it.a.limb(1, i, N), *b0 = it.b.limb(0, i, N), *b1 = it.b.limb(1, i, N);
    const u64 *pl = (it.add && p == 0) ? it.add + (size_t)i * N : nullptr;
    u64 *o = it.dst.limb(p, i, N);
    u64 base[E];
    if (p == 0) {
#pragma unroll
        for (int j = 0; j < E; j++) base[j] = mulmod(a0[g[j]], b0[g[j]], M);
        if (pl) {
#pragma unroll
            for (int j = 0; j < E; j++) base[j] = addmod(base[j], pl[g[j]], M.q);
        }
    } else {
#pragma unroll
        for (int j = 0; j < E; j++) {
            Acc128 t;
            t.clear();
            t.mac(a0[g[j]], b1[g[j]]);
            t.mac(a1[g[j]], b0[g[j]]);
            base[j] = t.reduce(M);
        }
    }
#pragma unroll
    for (int j = 0; j < E; j++) {
        v[j] = submod(mulmod(addmod(mulmod(ac[g[j]], pinv, M), base[j], M.q), k1, M), x[j], M.q);
        o[g[j]] = v[j];
    }
}

// grid = (tiles, 2B * cnt), z = (b*2 + p)*cnt + i with cnt = l - 1; CONT_MUL / CONT_BOOT (grid (tiles, B * cnt), z = b*cnt + i) carry on into the
// consumer's first phase exactly as f_frows_final_cont_kernel's rescale forms do: the merged step keeps the rescale's outgoing hand-off.
template <int K, int LOGE, int CONT>
__global__ __launch_bounds__(kTileThreads) void f_frows_fold_final_kernel(const u64 *__restrict__ tmp, const MulRsItem *__restrict__ items,
                                                                           const u64 *__restrict__ acc, int ell, int Kp,
                                                                           const DModulus *__restrict__ mods, const u64 *__restrict__ inv_last,
                                                                           const u64 *__restrict__ tw, const u64 *__restrict__ itw, int logN,
                                                                           Handoff h)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    constexpr int E = 1 << LOGE, NP = num_passes<LOGE>(K);
    const size_t N = (size_t)1 << logN;
    const int cnt = ell - 1;
    int g[E];
#pragma unroll
    for (int j = 0; j < E; j++) g[j] = tile_gidx<K, LOGE, false>(NP - 1, logN, blockIdx.x, j);
    auto nold = [](int) -> u64 { return 0; };
    if (CONT == CONT_BOOT) {
        const int z = blockIdx.y, i = z % cnt, b = z / cnt;
        const DModulus M = mods[i];
        const MulRsItem it = items[b];
        u64 v0[E], v1[E];
        fold_final_value<K, LOGE>(v0, g, tmp + ((size_t)(b * 2 + 0) * cnt + i) * N, it, acc, b, 0, i, ell, Kp, M, inv_last, tw, logN, lds);
        __syncthreads(); // the tile's last LDS image has been read by everyone
        fold_final_value<K, LOGE>(v1, g, tmp + ((size_t)(b * 2 + 1) * cnt + i) * N, it, acc, b, 1, i, ell, Kp, M, inv_last, tw, logN, lds);
        const u64 *sk = h.sk + (size_t)i * N;
#pragma unroll
        for (int j = 0; j < E; j++) v0[j] = addmod(v0[j], mulmod(v1[j], sk[g[j]], M), M.q);
        __syncthreads();
        u64 *o = h.out + (size_t)z * N;
        ntt_tile_x<K, LOGE, false, true, false, true, false>(v0, M, itw + ((size_t)i << logN), logN, blockIdx.x, nold, [=](int gi, u64 v) { o[gi] = v; }, lds);
    } else {
        const int z = blockIdx.y, i = z % cnt, bp = z / cnt, b = bp >> 1, p = bp & 1;
        const DModulus M = mods[i];
        u64 v[E];
        fold_final_value<K, LOGE>(v, g, tmp + (size_t)z * N, items[b], acc, b, p, i, ell, Kp, M, inv_last, tw, logN, lds);
        if (CONT == CONT_MUL) {
            if (p != 1) return;
            const CtView other = h.other[b];
            if (other.p) {
                const u64 *o1 = other.limb(1, i, N);
#pragma unroll
                for (int j = 0; j < E; j++) v[j] = mulmod(v[j], o1[g[j]], M);
            } else {
#pragma unroll
                for (int j = 0; j < E; j++) v[j] = mulmod(v[j], v[j], M);
            }
            __syncthreads();
            u64 *o = h.out + ((size_t)b * cnt + i) * N;
            ntt_tile_x<K, LOGE, false, true, false, true, false>(v, M, itw + ((size_t)i << logN), logN, blockIdx.x, nold, [=](int gi, u64 y) { o[gi] = y; }, lds);
        }
    }
}

// L3 + L4 + L5 in one launch (latency path): grid = (tiles, l + 2, B).  Workgroup (tile, y, b) owns one ROWS-phase tile of
// output modulus slot m (y < l: prime y, both accumulators; y = l, l + 1: the special prime, accumulator y - l).  For every
// digit j it finishes the NTT of the lifted digit (forward ROWS phase, result kept in registers) -- or, for j == m, reads the
// operand itself, which is already in NTT form -- and multiplies by the key limb at the same coefficients.  The special-prime
// accumulators continue in registers into the inverse ROWS phase that the mod-down starts with.
// MODE 0: rotation (operand = c1 of the item through its Galois permutation, key per item); MODE 1: relinearisation.
// FOLD (MODE 1, option ks_fold_rescale; items is a MulRsItem table, pmod = P mod q_i): the multiply's rescale is folded into the key switch.
// Row l - 1 -- the limb that rescale drops -- starts its accumulators at P (d + A) (d the tensor term, A the plaintext added to c0) and leaves,
// like the special prime's, as the first inverse ROWS phase of both accumulators, in its own slot of acc: f_dr2_icols_lift_fcols_kernel
// divides by P and by q_{l-1} in one pass from the two.
template <int K, int LOGE, int MODE, bool MERGE, bool FOLD = false>
__global__ __launch_bounds__(kTileThreads) void f_ks_frows_mac_kernel(const u64 *__restrict__ ext, const u64 *__restrict__ target,
                                                                       const KsItem *__restrict__ items,
                                                                       const u64 *__restrict__ shared_key, u64 *__restrict__ acc, int ell,
                                                                       int Kp, const DModulus *__restrict__ mods,
                                                                       const u64 *__restrict__ tw, const u64 *__restrict__ itw, int logN,
                                                                       const u64 *__restrict__ pmod, int items_fast)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    constexpr int E = 1 << LOGE, NP = num_passes<LOGE>(K);
    // ks_row's decode (ks_mac.hpp: the items-fast grid order, MERGE and psel are described there), written out: through the function the compiler
    // settles the comparison of y with l before it has seen this kernel's own tests of m, and every instantiation's code changes
    const int y = items_fast ? blockIdx.z : blockIdx.y, b = items_fast ? blockIdx.y : blockIdx.z, sp = Kp - 1;
    const int m = y < ell ? y : ell, psel = (MERGE && y == ell) ? -1 : y - ell;
    const int pm = m == ell ? sp : m;
    const size_t N = (size_t)1 << logN;
    const DModulus M = mods[pm];
    const u64 *key = MODE == 0 ? items[b].key : shared_key;
    int g[E];
#pragma unroll
    for (int e = 0; e < E; e++) g[e] = tile_gidx<K, LOGE, false>(NP - 1, logN, blockIdx.x, e);
    Acc128 a0[E], a1[E];
#pragma unroll
    for (int e = 0; e < E; e++) a0[e].clear(), a1[e].clear();
    if (MODE == 0 && pmod && m < ell) {
        // A rotation's base term rides on the accumulator: galois(c0) + (acc - t) P^-1 = ((acc + P galois(c0)) - t) P^-1 exactly, so the last
        // kernel of the key switch has no gather to do (this one has the Galois map in hand for c1 anyway).  The residue P galois(c0) mod q
        // is the accumulator's START value -- below 2^60 like a folded window, so the 16-products-per-window bound is unchanged -- and it is
        // computed here, before anything else is live (added in the epilogue it cost the merged form 6 VGPRs and a wave per SIMD).
        const KsItem &it = items[b];
        const u64 *c0 = it.src.limb(0, m, N);
        const u64 P = pmod[m];
        u64 cv[E];
        galois_gather<E>(cv, c0, (u32)g[0], it.elt, logN);
        if (it.add.p) {
            // ... and so does an addend y at the hop's level (option ks_fold_add: y' = y + rotate(y, o) as ONE key switch).  P y = 0 modulo the
            // special prime, so the mod-down's term t is unchanged and ((acc + P (galois(c0) + y0)) - t) P^-1 = galois(c0) + y0 + (acc - t) P^-1,
            // likewise y1 on the other accumulator: the limbs of "rotate, then add".  Both start values are canonical residues (the bound
            // above holds as it is).  A ROWS tile leaves a thread the consecutive coefficients g[0] + e: y is read as 16-byte vectors, no map.
            const u64 *y0 = it.add.limb(0, m, N) + g[0], *y1 = it.add.limb(1, m, N) + g[0];
#pragma unroll
            for (int e = 0; e < E; e += 2) {
                const u64x2 v0 = *reinterpret_cast<const u64x2 *>(y0 + e), v1 = *reinterpret_cast<const u64x2 *>(y1 + e);
                a0[e].lo = mulmod(addmod(cv[e], v0.x, M.q), P, M), a0[e + 1].lo = mulmod(addmod(cv[e + 1], v0.y, M.q), P, M);
                a1[e].lo = mulmod(v1.x, P, M), a1[e + 1].lo = mulmod(v1.y, P, M);
            }
        } else {
#pragma unroll
            for (int e = 0; e < E; e++) a0[e].lo = mulmod(cv[e], P, M);
        }
    }
    if (FOLD && m == ell - 1) { // (start values for the reason given above: nothing else is live yet)
        const MulRsItem &it = reinterpret_cast<const MulRsItem *>(items)[b];
        const u64 *pa0 = it.a.limb(0, m, N), *pa1 = it.a.limb(1, m, N), *pb0 = it.b.limb(0, m, N), *pb1 = it.b.limb(1, m, N);
        const u64 *pl = it.add ? it.add + (size_t)m * N : nullptr;
        const u64 P = pmod[m];
#pragma unroll
        for (int e = 0; e < E; e++) {
            const u64 va0 = pa0[g[e]], va1 = pa1[g[e]], vb0 = pb0[g[e]], vb1 = pb1[g[e]];
            u64 d0 = mulmod(va0, vb0, M);
            if (pl) d0 = addmod(d0, pl[g[e]], M.q);
            Acc128 t;
            t.clear();
            t.mac(va0, vb1);
            t.mac(va1, vb0);
            a0[e].lo = mulmod(d0, P, M), a1[e].lo = mulmod(t.reduce(M), P, M);
        }
    }
    auto nost = [](int, u64) {};
    auto nold = [](int) -> u64 { return 0; };
    bool lds_used = false;
    // Latency-shaped launches (not MERGE; one or two workgroups per CU, each walking its digits serially): the walk is software-pipelined.
    //   * the tile's twiddles are the same for every digit (same prime, same tile): fetched once (tile_twiddles), not once per transform
    //   * digit j + 1's coefficients and digit j's key limbs are requested BEFORE digit j's transform: the loads fly under its passes
    // so that a digit costs its butterflies and LDS exchanges, not a memory round trip before and another after them.  The extra live
    // registers (twiddles, next coefficients, key limbs) do not cost occupancy where this form runs: such launches have at most two waves per SIMD.
    constexpr bool PF = !MERGE && LOGE <= 2;
    u64 wtw[PF ? NP : 1][E];
    // a ROWS tile's first forward pass holds coefficients gin0 + e * SUBT, its last pass leaves g[0] + e (PassMap::idx_of)
    constexpr int SUBT = (1 << K) >> LOGE;
    int gin0 = 0;
    if (PF) {
        tile_twiddles<K, PF ? LOGE : 1, false, false>(reinterpret_cast<u64 (&)[num_passes<PF ? LOGE : 1>(K)][1 << (PF ? LOGE : 1)]>(wtw), tw + ((size_t)pm << logN),
                                                      logN, blockIdx.x);
        gin0 = tile_gidx<K, LOGE, false>(0, logN, blockIdx.x, 0);
    }
    // digit j's operand at this tile: its own limb (j == m: NTT form already, thread <-> coefficient map g) or the raised limb's first-pass image
    auto own_on_the_fly = [&](int j) { return j == m && MODE != 0 && !target; };
    auto fetch_x = [&](int j, u64 (&x)[E]) {
        const bool own = j == m;
        if (MODE == 0 && own) {
            const KsItem &it = items[b];
            galois_gather<E>(x, it.src.limb(1, j, N), (u32)g[0], it.elt, logN);
        } else if (!own || target) { // (one load path with a selected base and stride: two index arrays made the compiler select between them in memory)
            const u64 *src = own ? target + ((size_t)b * ell + j) * N : ext + (((size_t)b * ell + j) * ell + (m < j ? m : m - 1)) * N;
            const int base = own ? g[0] : gin0, stride = own ? 1 : SUBT;
#pragma unroll
            for (int e = 0; e < E; e++) x[e] = src[base + e * stride];
        }
    };
    // (round 5, measured and not kept: TWO digits ahead -- digit j + 2's coefficients and digit j + 1's key limbs requested before digit j's
    // transform, +24 VGPRs -- does nothing for a 13-prime hop (84.9 against 84.6-86.1 us) and costs config 3 a workgroup per CU: its 1 664
    // workgroups at 178 VGPRs run 2 to a CU instead of 3, 459 against 430-443 us; profiles/r05_experiments.txt)
    u64 xn[E];
    if (PF) fetch_x(0, xn);
    for (int j = 0; j < ell; j++) {
        u64 x[E];
        const u64 *k0 = key + (((size_t)j * 2 + 0) * Kp + pm) * N, *k1 = key + (((size_t)j * 2 + 1) * Kp + pm) * N;
        u64 kv0[E], kv1[E];
        if (PF && psel != 1) {
#pragma unroll
            for (int e = 0; e < E; e++) kv0[e] = k0[g[e]];
        }
        if (PF && psel != 0) {
#pragma unroll
            for (int e = 0; e < E; e++) kv1[e] = k1[g[e]];
        }
        if (PF) {
#pragma unroll
            for (int e = 0; e < E; e++) x[e] = xn[e];
            if (j + 1 < ell) fetch_x(j + 1, xn);
            if (own_on_the_fly(j)) { // c2 = a1*b1 on the fly (items points at the MulItem table)
                const MulItem &it = FOLD ? static_cast<const MulItem &>(reinterpret_cast<const MulRsItem *>(items)[b]) : reinterpret_cast<const MulItem *>(items)[b];
                const u64 *a1 = it.a.limb(1, j, N), *b1 = it.b.limb(1, j, N);
#pragma unroll
                for (int e = 0; e < E; e++) x[e] = mulmod(a1[g[e]], b1[g[e]], M);
            } else if (j != m) {
                if (lds_used) __syncthreads(); // the previous tile's last LDS image has been read by everyone
                ntt_tile_x<K, LOGE, false, false, true, true, true>(x, M, tw + ((size_t)pm << logN), logN, blockIdx.x, nold, nost, lds,
                                                                    PF ? wtw : nullptr);
                lds_used = true;
            }
        } else if (j == m) {
            if (MODE == 0) {
                const KsItem &it = items[b];
                galois_gather<E>(x, it.src.limb(1, j, N), (u32)g[0], it.elt, logN);
            } else if (target) {
                const u64 *tg = target + ((size_t)b * ell + j) * N;
#pragma unroll
                for (int e = 0; e < E; e++) x[e] = tg[g[e]];
            } else { // c2 = a1*b1 on the fly (items points at the MulItem table)
                const MulItem &it = FOLD ? static_cast<const MulItem &>(reinterpret_cast<const MulRsItem *>(items)[b]) : reinterpret_cast<const MulItem *>(items)[b];
                const u64 *a1 = it.a.limb(1, j, N), *b1 = it.b.limb(1, j, N);
#pragma unroll
                for (int e = 0; e < E; e++) x[e] = mulmod(a1[g[e]], b1[g[e]], M);
            }
        } else {
            const u64 *in = ext + (((size_t)b * ell + j) * ell + (m < j ? m : m - 1)) * N;
            if (lds_used) __syncthreads(); // the previous tile's last LDS image has been read by everyone
            ntt_tile_x<K, LOGE, false, false, true, false, true>(x, M, tw + ((size_t)pm << logN), logN, blockIdx.x,
                                                                 [=](int gi) { return in[gi]; }, nost, lds);
            lds_used = true;
        }
        if (psel != 1) {
#pragma unroll
            for (int e = 0; e < E; e++) a0[e].mac(x[e], PF ? kv0[e] : k0[g[e]]);
        }
        if (psel != 0) {
#pragma unroll
            for (int e = 0; e < E; e++) a1[e].mac(x[e], PF ? kv1[e] : k1[g[e]]);
        }
        if ((j & 15) == 15 && j + 1 < ell) { // a 128-bit accumulator holds 16 products of canonical residues (Acc128): fold it into a word
#pragma unroll
            for (int e = 0; e < E; e++) { // (ks_fold, ks_mac.hpp, written out: through the function the generic-width build's code changes)
                const u64 f0 = a0[e].reduce(M), f1 = a1[e].reduce(M);
                a0[e].clear(), a1[e].clear();
                a0[e].lo = f0, a1[e].lo = f1; // the folded sum counts as one more (tiny) term: 16 products + 2^60 < 2^124
            }
        }
    }
    if (FOLD && m == ell - 1) {
        for (int p = 0; p < 2; p++) {
            u64 r[E];
#pragma unroll
            for (int e = 0; e < E; e++) r[e] = p == 0 ? a0[e].reduce(M) : a1[e].reduce(M);
            u64 *o = acc + (((size_t)b * 2 + p) * (ell + 1) + m) * N;
            if (lds_used) __syncthreads();
            ntt_tile_x<K, LOGE, false, true, false, true, false>(r, M, itw + ((size_t)pm << logN), logN, blockIdx.x, nold,
                                                                 [=](int gi, u64 v) { o[gi] = v; }, lds);
            lds_used = true;
        }
    } else if (m < ell) {
        u64 *ac = acc + (size_t)b * 2 * (ell + 1) * N;
        u64 *o0 = ac + ((size_t)0 * (ell + 1) + m) * N, *o1 = ac + ((size_t)1 * (ell + 1) + m) * N;
#pragma unroll
        for (int e = 0; e < E; e++) o0[g[e]] = a0[e].reduce(M), o1[g[e]] = a1[e].reduce(M);
    } else {
        const int p_lo = MERGE ? 0 : psel, p_hi = MERGE ? 1 : psel;
        for (int p = p_lo; p <= p_hi; p++) {
            u64 r[E];
#pragma unroll
            for (int e = 0; e < E; e++) r[e] = p == 0 ? a0[e].reduce(M) : a1[e].reduce(M);
            u64 *o = acc + (((size_t)b * 2 + p) * (ell + 1) + ell) * N;
            if (lds_used) __syncthreads();
            ntt_tile_x<K, LOGE, false, true, false, true, false>(r, M, itw + ((size_t)sp << logN), logN, blockIdx.x, nold,
                                                                 [=](int gi, u64 v) { o[gi] = v; }, lds);
            lds_used = true;
        }
    }
}

// opcode 10, third launch (source at 1 prime; with 2 the composition in the loader spills and the separate launches are
// faster): z = b*t + k.  The loader re-encodes coefficient g of item b from its decrypted
// coefficient-domain limbs (CRT compose, conjugate projection, scale, round), reduces it into target prime k, and the tile
// runs the first forward phase -- reencode_lift_batch_kernel + launch_ntt_cols_fwd without the round trip through ptx.
template <int K, int LOGE, int ELL>
__global__ __launch_bounds__(kTileThreads) void f_boot_reencode_fcols_kernel(const u64 *__restrict__ pt, u64 *__restrict__ ptx,
                                                                              const BootItem *__restrict__ items, int t,
                                                                              const DModulus *__restrict__ mods, const CrtDev crt,
                                                                              const u64 *__restrict__ tw, int logN)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    const int z = blockIdx.y, k = z % t, b = z / t;
    const size_t N = (size_t)1 << logN;
    const double ratio = items[b].ratio;
    const u64 *cf = pt + (size_t)b * ELL * N;
    u64 *out = ptx + (size_t)z * N;
    const DModulus M = mods[k];
    ntt_tile<K, LOGE, true, false, false>(
        M, tw + ((size_t)k << logN), logN, blockIdx.x,
        [=](int g) { return residue_of_double(reencoded_coeff_fixed<ELL>(cf, (size_t)g, N, mods, crt, ratio), M); },
        [=](int g, u64 v) { out[g] = v; }, lds);
}

// opcode 10, last launch: z = b*t + i.  dst.c0 = zenc.c0 + NTT(re-encoded plaintext), dst.c1 = zenc.c1
template <int K, int LOGE>
__global__ __launch_bounds__(kTileThreads) void f_frows_boot_final_kernel(const u64 *__restrict__ ptx, const BootItem *__restrict__ items,
                                                                           int t, const DModulus *__restrict__ mods,
                                                                           const u64 *__restrict__ tw, int logN)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    const int z = blockIdx.y, i = z % t;
    const size_t N = (size_t)1 << logN;
    const BootItem it = items[z / t];
    const DModulus M = mods[i];
    const u64 *in = ptx + (size_t)z * N;
    const u64 *z0 = it.zenc + (size_t)i * N, *z1 = it.zenc + ((size_t)t + i) * N;
    u64 *o0 = it.dst.limb(0, i, N), *o1 = it.dst.limb(1, i, N);
    ntt_tile<K, LOGE, false, false, true>(
        M, tw + ((size_t)i << logN), logN, blockIdx.x, [=](int g) { return in[g]; },
        [=](int g, u64 v) {
            o0[g] = addmod(v, z0[g], M.q);
            o1[g] = z1[g];
        },
        lds);
}

// ---- launchers (K and geometry dispatch: tile_dispatch.hpp) ---------------------------------------------------------------
template <class Src>
static void launch_irows(const Context &c, Src src, u64 *out, long out_stride, int count, hipStream_t s)
{
    DC_GEO_SWITCH(c.k2, count, DC_LAUNCH((f_irows_kernel<KK, LE, Src>), grid, dim3(kTileThreads), 0, s, src, out, out_stride,
                                                  c.d_mods, c.d_itw, c.logN));
}

void f_irows_strided(const Context &c, const u64 *base, long stride, int prime_base, int period, u64 *out, long out_stride, int count,
                     hipStream_t s)
{
    launch_irows(c, SrcStrided{ base, stride, prime_base, period }, out, out_stride, count, s);
}
// L1 of a rotation batch: inverse ROWS phase of galois(c1).  z = b*l + j.  An inverse ROWS tile starts with 2^LOGE CONSECUTIVE coefficients per
// thread, so the Galois gather is 16-byte loads of aligned pairs (galois_gather) instead of one 8-byte load per coefficient through a loader
// functor (the geometries with at least two coefficients per thread: all three)
template <int K, int LOGE>
__global__ __launch_bounds__(kTileThreads) void f_irows_rot_kernel(const KsItem *__restrict__ items, int ell, u64 *__restrict__ out,
                                                                    const DModulus *__restrict__ mods, const u64 *__restrict__ itw, int logN)
{
    __shared__ __attribute__((aligned(16))) u64 lds[TileGeo<LOGE>::LDS_ELEMS];
    constexpr int E = 1 << LOGE;
    const int z = blockIdx.y, j = z % ell;
    const size_t N = (size_t)1 << logN;
    const KsItem &it = items[z / ell];
    u64 *o = out + (size_t)z * N;
    u64 x[E];
    galois_gather<E>(x, it.src.limb(1, j, N), (u32)tile_gidx<K, LOGE, false>(num_passes<LOGE>(K) - 1, logN, blockIdx.x, 0), it.elt, logN);
    auto nold = [](int) -> u64 { return 0; };
    ntt_tile_x<K, LOGE, false, true, false, true, false>(x, mods[j], itw + ((size_t)j << logN), logN, blockIdx.x, nold,
                                                         [=](int gi, u64 v) { o[gi] = v; }, lds);
}

void f_irows_rot_c1(const Context &c, const KsItem *items, int ell, u64 *out, int B, hipStream_t s)
{
    DC_GEO_SWITCH(c.k2, B * ell, DC_LAUNCH((f_irows_rot_kernel<KK, LE>), grid, dim3(kTileThreads), 0, s, items, ell, out, c.d_mods, c.d_itw,
                                                    c.logN));
}
void f_irows_rs_last(const Context &c, const RsItem *items, const SumSrc *srcs, int l, u64 *out, int B, hipStream_t s)
{
    DC_GEO_SWITCH(c.k2, 2 * B, DC_LAUNCH((f_irows_rs_kernel<KK, LE>), grid, dim3(kTileThreads), 0, s, items, srcs, l, out, c.d_mods,
                                                  c.d_itw, c.logN));
}
void f_irows_rs_single(const Context &c, CtView src, int l, u64 *out, hipStream_t s)
{
    launch_irows(c, SrcRsLast1{ src, l }, out, (long)c.N, 2, s);
}
void f_irows_decrypt(const Context &c, CtView ct, const u64 *sk, int ell, u64 *out, hipStream_t s)
{
    launch_irows(c, SrcDecrypt{ ct, sk, c.d_mods }, out, (long)c.N, ell, s);
}

void f_irows_tensor_c2(const Context &c, const MulItem *items, int ell, u64 *out, int B, hipStream_t s)
{
    launch_irows(c, SrcTensorC2<MulItem>{ items, c.d_mods, ell }, out, (long)c.N, B * ell, s);
}
void f_irows_tensor_c2_rs(const Context &c, const MulRsItem *items, int ell, u64 *out, int B, hipStream_t s)
{
    launch_irows(c, SrcTensorC2<MulRsItem>{ items, c.d_mods, ell }, out, (long)c.N, B * ell, s);
}
void f_irows_tensor_sum(const Context &c, const MulSumItem *items, const MulTerm *terms, int ell, u64 *out, u64 *target, int B, hipStream_t s)
{
    DC_GEO_SWITCH(c.k2, B * ell, DC_LAUNCH((f_irows_tensor_sum_kernel<KK, LE>), grid, dim3(kTileThreads), 0, s, items, terms, ell, out, target,
                                                    c.d_mods, c.d_itw, c.logN));
}
void f_frows_sum_final(const Context &c, const u64 *tmp, const MulSumItem *items, const MulTerm *terms, const u64 *acc, int B, int ell, hipStream_t s)
{
    const int sp = c.K - 1;
    if (terms) {
        DC_GEO_SWITCH(c.k2, 2 * B * ell, DC_LAUNCH((f_frows_sum_final_kernel<KK, LE, true>), grid, dim3(kTileThreads), 0, s, tmp, items, terms, acc,
                                                            ell, sp, c.K, c.d_mods, c.d_inv_last, c.d_tw, c.logN));
    } else {
        DC_GEO_SWITCH(c.k2, 2 * B * ell, DC_LAUNCH((f_frows_sum_final_kernel<KK, LE, false>), grid, dim3(kTileThreads), 0, s, tmp, items, terms, acc,
                                                            ell, sp, c.K, c.d_mods, c.d_inv_last, c.d_tw, c.logN));
    }
}
void f_irows_decrypt_items(const Context &c, const BootItem *items, const SumSrc *srcs, const u64 *sk, int ell, u64 *out, int B,
                           hipStream_t s)
{
    DC_GEO_SWITCH(c.k2, B * ell, DC_LAUNCH((f_irows_boot_kernel<KK, LE>), grid, dim3(kTileThreads), 0, s, items, srcs, sk, ell, out,
                                                    c.d_mods, c.d_itw, c.logN));
}
void f_boot_reencode_fcols(const Context &c, const u64 *pt, u64 *ptx, const BootItem *items, int B, int ell, int t, CrtDev crt,
                           hipStream_t s)
{
    if (ell == 1) {
        DC_GEO_SWITCH(c.k1, B * t, DC_LAUNCH((f_boot_reencode_fcols_kernel<KK, LE, 1>), grid, dim3(kTileThreads), 0, s, pt, ptx, items,
                                                      t, c.d_mods, crt, c.d_tw, c.logN));
    } else {
        fprintf(stderr, "[dacapo_amd] f_boot_reencode_fcols: source level %d not instantiated\n", ell);
        abort();
    }
}
void f_frows_boot_final(const Context &c, const u64 *ptx, const BootItem *items, int B, int t, hipStream_t s)
{
    DC_GEO_SWITCH(c.k2, B * t, DC_LAUNCH((f_frows_boot_final_kernel<KK, LE>), grid, dim3(kTileThreads), 0, s, ptx, items, t,
                                                  c.d_mods, c.d_tw, c.logN));
}

// (launch shape: ks_mac.hpp ks_mac_shape)
void f_ks_frows_mac(const Context &c, int mode, const u64 *ext, const u64 *target, const KsItem *items, const u64 *shared_key, u64 *acc,
                    int B, int ell, hipStream_t s, bool fold_base)
{
    const u64 *pmod = (fold_base && mode == 0) ? c.d_pmod : nullptr;
    const KsMacShape sh = ks_mac_shape(c, ell, B);
    ks_mac_dispatch(c.k2, sh, [&](auto k, auto le, auto merge) {
        constexpr int KK = decltype(k)::value, LE = decltype(le)::value;
        constexpr bool MG = decltype(merge)::value;
        if (mode == 0)
            DC_LAUNCH((f_ks_frows_mac_kernel<KK, LE, 0, MG>), sh.grid, dim3(kTileThreads), 0, s, ext, target, items, shared_key, acc, ell, c.K,
                      c.d_mods, c.d_tw, c.d_itw, c.logN, pmod, sh.items_fast);
        else
            DC_LAUNCH((f_ks_frows_mac_kernel<KK, LE, 1, MG>), sh.grid, dim3(kTileThreads), 0, s, ext, target, items, shared_key, acc, ell, c.K,
                      c.d_mods, c.d_tw, c.d_itw, c.logN, pmod, sh.items_fast);
    });
}

void f_ks_frows_mac_rs(const Context &c, const u64 *ext, const MulRsItem *items, const u64 *relin_key, u64 *acc, int B, int ell, hipStream_t s)
{
    const KsMacShape sh = ks_mac_shape(c, ell, B);
    ks_mac_dispatch(c.k2, sh, [&](auto k, auto le, auto merge) {
        constexpr int KK = decltype(k)::value, LE = decltype(le)::value;
        constexpr bool MG = decltype(merge)::value;
        DC_LAUNCH((f_ks_frows_mac_kernel<KK, LE, 1, MG, true>), sh.grid, dim3(kTileThreads), 0, s, ext, nullptr, reinterpret_cast<const KsItem *>(items),
                  relin_key, acc, ell, c.K, c.d_mods, c.d_tw, c.d_itw, c.logN, c.d_pmod, sh.items_fast);
    });
}

static long ks_merge_lift_min_wgs()
{ // option ks_merge_lift_min_wgs: launches of L2 / L6 that still have at least this many workgroups AFTER merging share the inverse COLS
  // phase among a source limb's target moduli (a single key switch at 13 primes has 5408 fine workgroups or 416 merged ones: merged it
  // leaves CUs idle, 115 us against 93); a huge value = never
    return (long)option(OPT_KS_MERGE_LIFT_MIN_WGS);
}
// L2 / L6 / R2: `sources` source limbs with `per_source` target moduli each.  launch(K, LE, MERGE, grid) with the first three as
// std::integral_constant values; grid.y = the limbs, or the sources when merged.
// (the tile geometry is chosen from the unmerged limb count either way: the merged form is a throughput form of the same launch)
template <class Launch>
static void merged_dispatch(const Context &c, int sources, int per_source, Launch launch)
{
    const int limbs = sources * per_source, le = tile_geo_le(c.N, limbs);
    const unsigned tiles = (unsigned)(c.N >> tile_geo_log(le));
    const bool merge = per_source > 1 && (long)tiles * sources >= ks_merge_lift_min_wgs();
    const dim3 grid(tiles, (unsigned)(merge ? sources : limbs));
    tile_dispatch(c.k1, le, [&](auto k, auto le_c) {
        if (merge)
            launch(k, le_c, std::true_type{}, grid);
        else
            launch(k, le_c, std::false_type{}, grid);
    });
}

void f_ks_icols_lift_fcols(const Context &c, const u64 *digits, u64 *ext, int B, int ell, hipStream_t s)
{
    merged_dispatch(c, B * ell, ell, [&](auto k, auto le, auto merge, dim3 grid) {
        DC_LAUNCH((f_ks_icols_lift_fcols_kernel<k(), le(), merge()>), grid, dim3(kTileThreads), 0, s, digits, ext, ell, c.K - 1, c.d_mods, c.d_tw,
                  c.d_itw, c.logN, c.twc2());
    });
}

// (noise: the byte noise of zero-encryptions, f_dr_noise_icols_lift_fcols; null = the plain divide-and-round)
template <bool NOISE>
static void launch_dr_icols_lift_fcols(const Context &c, const u64 *last, long last_stride, u64 *tmp, int polys, int cnt, int l,
                                       const signed char *noise, hipStream_t s)
{
    merged_dispatch(c, polys, cnt, [&](auto k, auto le, auto merge, dim3 grid) {
        DC_LAUNCH((f_dr_icols_lift_fcols_kernel<k(), le(), merge(), NOISE>), grid, dim3(kTileThreads), 0, s, last, last_stride, tmp, cnt, l, c.K,
                  c.d_mods, c.d_half_mod, c.d_tw, c.d_itw, c.logN, c.twc2(), noise);
    });
}
void f_dr_icols_lift_fcols(const Context &c, const u64 *last, long last_stride, u64 *tmp, int polys, int cnt, int l, hipStream_t s)
{
    launch_dr_icols_lift_fcols<false>(c, last, last_stride, tmp, polys, cnt, l, nullptr, s);
}
void f_dr_noise_icols_lift_fcols(const Context &c, const u64 *last, long last_stride, u64 *tmp, int polys, int cnt, int l,
                                 const signed char *noise, hipStream_t s)
{
    launch_dr_icols_lift_fcols<true>(c, last, last_stride, tmp, polys, cnt, l, noise, s);
}

void f_irows_zenc(const Context &c, const ZencItem *items, const u64 *pk, int l, u64 *out, int B, hipStream_t s)
{
    DC_GEO_SWITCH(c.k2, 2 * B, DC_LAUNCH((f_irows_zenc_kernel<KK, LE>), grid, dim3(kTileThreads), 0, s, items, pk, (long)c.K * (long)c.N, l, out,
                                                  c.d_mods, c.d_itw, c.logN));
}
void f_frows_zenc_final(const Context &c, const u64 *tmp, const ZencItem *items, const u64 *pk, int B, int l, hipStream_t s)
{
    DC_GEO_SWITCH(c.k2, 2 * B * l, DC_LAUNCH((f_frows_zenc_final_kernel<KK, LE>), grid, dim3(kTileThreads), 0, s, tmp, items, pk,
                                                      (long)c.K * (long)c.N, l, c.K, c.d_mods, c.d_inv_last, c.d_tw, c.logN));
}

void f_dr2_icols_lift_fcols(const Context &c, const u64 *acc, const MulRsItem *items, u64 *tmp, int B, int ell, hipStream_t s)
{
    merged_dispatch(c, 2 * B, ell - 1, [&](auto k, auto le, auto merge, dim3 grid) {
        DC_LAUNCH((f_dr2_icols_lift_fcols_kernel<k(), le(), merge()>), grid, dim3(kTileThreads), 0, s, acc, items, tmp, ell, c.K, c.d_mods,
                  c.d_half_mod, c.d_inv_last, c.d_tw, c.d_itw, c.logN, c.twc2());
    });
}

void f_frows_fold_final(const Context &c, const u64 *tmp, const MulRsItem *items, const u64 *acc, int B, int ell, hipStream_t s, const Handoff &h)
{
    const int cnt = ell - 1, groups = h.cont == CONT_BOOT ? B : 2 * B;
#define DC_FOLD(CT)                                                                                                                    \
    DC_GEO_SWITCH(c.k2, groups * cnt, DC_LAUNCH((f_frows_fold_final_kernel<KK, LE, CT>), grid, dim3(kTileThreads), 0, s, tmp, items, acc, ell, c.K, \
                                                         c.d_mods, c.d_inv_last, c.d_tw, c.d_itw, c.logN, h))
    switch (h.cont) {
    case CONT_NONE: DC_FOLD(CONT_NONE); break;
    case CONT_MUL: DC_FOLD(CONT_MUL); break;
    case CONT_BOOT: DC_FOLD(CONT_BOOT); break;
    default: fprintf(stderr, "[dacapo_amd] f_frows_fold_final: no continuation kernel for consumer kind %d\n", h.cont); abort();
    }
#undef DC_FOLD
}

void f_ks_lift_fcols(const Context &c, const u64 *digits, u64 *ext, int B, int ell, hipStream_t s)
{
    if ((c.k1 == 7 || c.k1 == 8) && use_wide_tiles(c.N, (long)B * ell * ell) && !use_small_tiles(c.N, (long)B * ell * ell)) { // round 5: radix-16 COLS tiles
        constexpr int LE = 4;                                                                                               // (ntt_tile.hpp; two phase sizes instantiated)
        const dim3 grid((unsigned)(c.N >> TileGeo<LE>::LOG), (unsigned)(B * ell * ell));
        if (c.k1 == 7)
            DC_LAUNCH((f_ks_lift_fcols_kernel<7, LE>), grid, dim3(kTileThreads), 0, s, digits, ext, ell, c.K - 1, c.d_mods, c.d_tw, c.logN, c.twc2());
        else
            DC_LAUNCH((f_ks_lift_fcols_kernel<8, LE>), grid, dim3(kTileThreads), 0, s, digits, ext, ell, c.K - 1, c.d_mods, c.d_tw, c.logN, c.twc2());
        return;
    }
    DC_GEO_SWITCH(c.k1, B * ell * ell, DC_LAUNCH((f_ks_lift_fcols_kernel<KK, LE>), grid, dim3(kTileThreads), 0, s, digits, ext, ell,
                                                          c.K - 1, c.d_mods, c.d_tw, c.logN, c.twc2()));
}

void f_dr_lift_fcols(const Context &c, const u64 *last, long last_stride, u64 *tmp, int polys, int cnt, int l, hipStream_t s)
{
    DC_GEO_SWITCH(c.k1, polys * cnt, DC_LAUNCH((f_dr_lift_fcols_kernel<KK, LE>), grid, dim3(kTileThreads), 0, s, last, last_stride,
                                                        tmp, cnt, l, c.K, c.d_mods, c.d_half_mod, c.d_tw, c.logN, c.twc2()));
}

void f_frows_final(const Context &c, int mode, const u64 *tmp, const void *items, const u64 *acc, int polys, int cnt, int l,
                   hipStream_t s, RsItem single, const u64 *plain, const SumSrc *srcs, const Handoff &h, bool base_folded)
{
    const int folded = base_folded ? 1 : 0;
    if (h.cont != CONT_NONE) {
        const int groups = h.cont == CONT_BOOT ? polys / 2 : polys; // CONT_BOOT: one workgroup per (item, limb) does both polynomials
#define DC_CONT(MD, CT)                                                                                                                \
    DC_GEO_SWITCH(c.k2, groups * cnt, DC_LAUNCH((f_frows_final_cont_kernel<KK, LE, MD, CT>), grid, dim3(kTileThreads), 0, s, tmp, items, \
                                                         srcs, acc, cnt, l, c.K, c.d_mods, c.d_inv_last, c.d_tw, c.d_itw, c.logN, h, folded))
        if (mode == 4 && h.cont == CONT_RS) {
            DC_CONT(4, CONT_RS);
        } else if (mode == 2 && h.cont == CONT_MUL) {
            DC_CONT(2, CONT_MUL);
        } else if (mode == 2 && h.cont == CONT_BOOT) {
            DC_CONT(2, CONT_BOOT);
        } else if (mode == 0 && h.cont == CONT_BOOT) {
            DC_CONT(0, CONT_BOOT);
        } else {
            fprintf(stderr, "[dacapo_amd] f_frows_final: no continuation kernel for mode %d -> consumer kind %d\n", mode, h.cont);
            abort();
        }
#undef DC_CONT
        return;
    }
#define DC_FINAL(MD)                                                                                                                   \
    DC_GEO_SWITCH(c.k2, polys * cnt, DC_LAUNCH((f_frows_final_kernel<KK, LE, MD>), grid, dim3(kTileThreads), 0, s, tmp, items, single, \
                                                        plain, srcs, acc, cnt, l, c.K, c.d_mods, c.d_inv_last, c.d_tw, c.logN, folded))
    switch (mode) {
    case 0: DC_FINAL(0); break;
    case 1: DC_FINAL(1); break;
    case 2: DC_FINAL(2); break;
    case 4: DC_FINAL(4); break;
    default: DC_FINAL(3); break;
    }
#undef DC_FINAL
}

} // namespace dacapo
