// Sums of signed ct x ct products at a tile's coefficients (plan.hpp MulSumItem / MulTerm): what the first and the last kernel of a lazy
// relinearisation walk, under either key layout (fused_ks.hip f_irows_tensor_sum_kernel / f_frows_sum_final_kernel, hybrid_fused.hip
// hybf_irows_tensor_sum_kernel / hybf_frows_sum_final_kernel).
#pragma once
#include "plan.hpp"

namespace dacapo {

// tensor_sum's fold between two windows of 8 terms (either accumulator restarts from its canonical residue) and its last line, as functions
// for tensor_sum_rows.  (tensor_sum itself keeps them written out: called through these, f_frows_sum_final_kernel<.., true> of the SEAL-layout
// sequence schedules differently in 24 instantiations, and that kernel stays the code object it was.)
template <int E>
__device__ __forceinline__ void tensor_sum_fold(Acc128 (&pos)[E], Acc128 (&neg)[E], const DModulus &M)
{
#pragma unroll
    for (int j = 0; j < E; j++) {
        const u64 fp = pos[j].reduce(M), fn = neg[j].reduce(M);
        pos[j].clear(), neg[j].clear();
        pos[j].lo = fp, neg[j].lo = fn;
    }
}
template <int E>
__device__ __forceinline__ void tensor_sum_finish(u64 (&v)[E], const Acc128 (&pos)[E], const Acc128 (&neg)[E], const DModulus &M)
{
#pragma unroll
    for (int j = 0; j < E; j++) v[j] = submod(pos[j].reduce(M), neg[j].reduce(M), M.q);
}

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

// The same sum -- the same accumulators, the same fold every 8 terms, the same bound -- for a thread whose E coefficients are CONSECUTIVE,
// g0 .. g0 + E - 1 (what the first inverse pass and the last forward pass of a ROWS tile leave a thread with; g0 a multiple of E): every
// stream is 16-byte loads, and term t + 1's loads are issued before term t's products, so a walk waits for one memory latency per term and
// not for two (table entry -> limbs is still dependent: the entry's own load rides one term ahead as well).  A grouped-digit key switch runs at
// N = 2^16 / 2^17, where these loads come from HBM.
template <int E, int COMP>
__device__ __forceinline__ void tensor_sum_rows_part(u64 (&v)[E], int g0, const MulTerm *__restrict__ terms, int first, int count, int i, size_t N,
                                                     const DModulus &M)
{
    static_assert(E % 2 == 0, "pairs of coefficients");
    constexpr int S = COMP == 1 ? 2 : 1; // products per term and coefficient
    struct Ops {
        u64x2 x[S][E / 2], y[S][E / 2];
        int sign;
    };
    auto fetch = [&](int t, Ops &o) {
        const MulTerm tm = terms[first + t];
        o.sign = tm.sign;
        const u64 *x0 = tm.a.limb(COMP == 2 ? 1 : 0, i, N) + g0, *y0 = tm.b.limb(COMP == 0 ? 0 : 1, i, N) + g0;
#pragma unroll
        for (int j = 0; j < E / 2; j++)
            o.x[0][j] = *reinterpret_cast<const u64x2 *>(x0 + 2 * j), o.y[0][j] = *reinterpret_cast<const u64x2 *>(y0 + 2 * j);
        if (COMP == 1) {
            const u64 *x1 = tm.a.limb(1, i, N) + g0, *y1 = tm.b.limb(0, i, N) + g0;
#pragma unroll
            for (int j = 0; j < E / 2; j++)
                o.x[S - 1][j] = *reinterpret_cast<const u64x2 *>(x1 + 2 * j), o.y[S - 1][j] = *reinterpret_cast<const u64x2 *>(y1 + 2 * j);
        }
    };
    Acc128 pos[E], neg[E];
#pragma unroll
    for (int j = 0; j < E; j++) pos[j].clear(), neg[j].clear();
    auto mac_all = [&](Acc128(&a)[E], const Ops &o) {
#pragma unroll
        for (int s = 0; s < S; s++)
#pragma unroll
            for (int j = 0; j < E; j++) a[j].mac(o.x[s][j >> 1][j & 1], o.y[s][j >> 1][j & 1]);
    };
    Ops nx;
    fetch(0, nx);
    for (int t = 0; t < count; t++) {
        const Ops cur = nx;
        if (t + 1 < count) fetch(t + 1, nx);
        if (cur.sign > 0) // (wave-uniform)
            mac_all(pos, cur);
        else
            mac_all(neg, cur);
        if ((t & 7) == 7 && t + 1 < count) tensor_sum_fold(pos, neg, M);
    }
    tensor_sum_finish(v, pos, neg, M);
}
// ... four coefficients at a time.  One walk over all 8 coefficients of a radix-8 tile's thread keeps 2 x 4 streams x 8 words in flight beside
// 16 accumulators: 284 .. 290 VGPRs in the last kernel (COMP 1), one wave per SIMD, and 196 in the first; two walks of 4 take 166 and 112,
// three and four waves (profiles/hyb_lazy_relin_regs.txt; compile-time figures, the two forms were not timed against each other).  The second walk's table entries and half of its limbs' lines are in cache.
template <int E, int COMP>
__device__ __forceinline__ void tensor_sum_rows(u64 (&v)[E], int g0, const MulTerm *__restrict__ terms, int first, int count, int i, size_t N,
                                                const DModulus &M)
{
    constexpr int C = E < 4 ? E : 4;
#pragma unroll
    for (int h = 0; h < E; h += C) {
        u64 part[C];
        tensor_sum_rows_part<C, COMP>(part, g0 + h, terms, first, count, i, N, M);
#pragma unroll
        for (int j = 0; j < C; j++) v[h + j] = part[j];
    }
}

} // namespace dacapo
