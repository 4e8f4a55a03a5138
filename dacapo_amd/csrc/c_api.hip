// Kernel-level C ABI (include/dacapo_ckks.h): thin extern "C" shims over the launchers.
#include "../../include/dacapo_ckks.h"

#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "kernels.hpp"
#include "noise_stats.hpp"
#include "plan.hpp"

using namespace dacapo;

#include "c_api_types.hpp"

static inline hipStream_t S(void *s) { return (hipStream_t)s; }
static inline CtView V(const uint64_t *p, long stride) { return CtView{ const_cast<u64 *>(p), stride }; }

// The composite ops run the same fused launch sequences as the HEVM execution plan (batch_ops.hip, fused_ks.hip) with a batch
// of one item; the item descriptor goes through a small ring of device slots, written in stream order.  Operands that alias
// the destination in a way the fused epilogues cannot tolerate fall back to the alias-safe unfused composites (ckks_ops.hip).
namespace {
constexpr int kItemSlots = 64;
constexpr size_t kItemBytes = 128;
static_assert(sizeof(KsItem) <= kItemBytes && sizeof(MulItem) <= kItemBytes && sizeof(RsItem) <= kItemBytes && sizeof(MulRsItem) <= kItemBytes, "item slot too small");
constexpr int kConstSlotWords = 64; // residues of one mul_const table (levels up to 64)
void *item_slot(dc_context *ctx, const void *host_item, size_t bytes, hipStream_t s)
{
    if (!ctx->item_ring) DC_HIP_CHECK(hipMalloc(&ctx->item_ring, kItemSlots * kItemBytes));
    char *slot = static_cast<char *>(ctx->item_ring) + (size_t)(ctx->item_next++ % kItemSlots) * kItemBytes;
    DC_HIP_CHECK(hipMemcpyAsync(slot, host_item, bytes, hipMemcpyHostToDevice, s));
    return slot;
}
BatchWs batch_ws(const Workspace &w) { return BatchWs{ w.ct_tmp, w.ks_digits, w.ks_ext, w.ks_acc, w.ks_tmp }; }
bool overlaps(const uint64_t *a, const uint64_t *b) { return a == b; }

// What the two hoisted entry points share.  A context with grouped digits is refused (`grouped`: why, in the entry point's words), count and level
// are checked, build(h) fills the host item table and returns how many decompositions need scratch in the handle; then the handle's buffers --
// the item table, `pairs` accumulator pairs with their mod-down terms, that scratch -- are grown on demand (growing waits for the device:
// hipFree) and the table is uploaded.  Returns the device table.
template <class Build>
const KsItem *hoist_items(dc_context *ctx, const char *who, const char *grouped, const char *what, int count, int ell, size_t pairs,
                                 hipStream_t s, Build build)
{
    Context &c = *ctx->c;
    if (c.hybrid()) {
        fprintf(stderr, "[dacapo_amd] %s: this context switches keys with grouped digits%s; the call is for SEAL-layout keys\n", who, grouped);
        abort();
    }
    if (count < 1 || count > 65535 || ell < 1 || ell > c.max_level()) {
        fprintf(stderr, "[dacapo_amd] %s: %d %s at level %d (1..65535 %s, level 1..%d)\n", who, count, what, ell, what, c.max_level());
        abort();
    }
    auto grow = [](auto *&p, size_t &cap, size_t need) {
        if (need <= cap) return;
        if (p) DC_HIP_CHECK(hipFree(p));
        p = nullptr;
        DC_HIP_CHECK(hipMalloc(&p, need));
        cap = need;
    };
    std::vector<KsItem> h;
    const size_t U = build(h), N = c.N;
    grow(ctx->hoist_items, ctx->hoist_item_cap, h.size() * sizeof(KsItem));
    grow(ctx->hoist_acc, ctx->hoist_acc_cap, pairs * 2 * ((size_t)ell + 1) * N * sizeof(u64));
    grow(ctx->hoist_tmp, ctx->hoist_tmp_cap, pairs * 2 * (size_t)ell * N * sizeof(u64));
    grow(ctx->hoist_digits, ctx->hoist_digits_cap, U * (size_t)ell * N * sizeof(u64));
    grow(ctx->hoist_ext, ctx->hoist_ext_cap, U * (size_t)ell * ell * N * sizeof(u64));
    DC_HIP_CHECK(hipMemcpyAsync(ctx->hoist_items, h.data(), h.size() * sizeof(KsItem), hipMemcpyHostToDevice, s));
    DC_HIP_CHECK(hipStreamSynchronize(s)); // (the host table goes out of scope)
    return static_cast<const KsItem *>(ctx->hoist_items);
}
} // namespace

extern "C" {

dc_context *dc_context_create(int logN, int num_primes, int bit_size, const uint64_t *primes)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        fprintf(stderr, "[dacapo_amd] no HIP device: the HEVM runtime has no CPU fallback\n");
        abort();
    }
    if (!primes && (bit_size < kMinQBits || bit_size > kQBits)) {
        fprintf(stderr, "[dacapo_amd] prime width %d outside %d..%d bits (the reference's chain is 60-bit, SEAL_HEVM.cpp:48-53)\n", bit_size, kMinQBits, kQBits);
        abort();
    }
    Context *c = new Context(logN, num_primes, bit_size, primes);
    c->ensure_scratch();
    return new dc_context{ c, true };
}
// EXTENSION: a context whose key switching uses grouped digits (hybrid_ks.hip): the last `special` primes are special, a digit is `alpha`
// data primes, keys passed to dc_ct_rotate_hop / dc_ct_mul_relin / dc_keyswitch are [ceil((K - special) / alpha)][2][K][N]
dc_context *dc_context_create_hybrid(int logN, int num_primes, int special, int alpha)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        fprintf(stderr, "[dacapo_amd] no HIP device: the HEVM runtime has no CPU fallback\n");
        abort();
    }
    Context *c = new Context(logN, num_primes, kQBits, nullptr, special, alpha);
    c->ensure_scratch();
    return new dc_context{ c, true };
}
// ... on an explicit chain (a HEaaN-style mixed one: 60-bit base and special primes around 51-bit rescale primes; the generic-width build)
dc_context *dc_context_create_hybrid_primes(int logN, const uint64_t *primes, int num_primes, int special, int alpha)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        fprintf(stderr, "[dacapo_amd] no HIP device: the HEVM runtime has no CPU fallback\n");
        abort();
    }
    Context *c = new Context(logN, num_primes, kQBits, primes, special, alpha);
    c->ensure_scratch();
    return new dc_context{ c, true };
}
int dc_context_key_digits(const dc_context *ctx) { return ctx->c->key_digits(); }
int dc_context_max_level(const dc_context *ctx) { return ctx->c->max_level(); }
void dc_context_destroy(dc_context *ctx)
{
    if (ctx && ctx->item_ring) (void)hipFree(ctx->item_ring);
    if (ctx)
        for (void *p : { ctx->hoist_items, (void *)ctx->hoist_acc, (void *)ctx->hoist_tmp, (void *)ctx->hoist_digits, (void *)ctx->hoist_ext, (void *)ctx->fold_consts,
                         (void *)ctx->fold_tmp, ctx->mulsum_table, (void *)ctx->noise_buf })
            if (p) (void)hipFree(p);
    if (ctx && ctx->owned) delete ctx->c;
    delete ctx;
}
int dc_context_logn(const dc_context *ctx) { return ctx->c->logN; }
int dc_context_num_primes(const dc_context *ctx) { return ctx->c->K; }
void dc_context_primes(const dc_context *ctx, uint64_t *out)
{
    for (int i = 0; i < ctx->c->K; i++) out[i] = ctx->c->primes[i];
}
void dc_context_roots(const dc_context *ctx, uint64_t *out)
{
    for (int i = 0; i < ctx->c->K; i++) out[i] = ctx->c->psi[i];
}

void *dc_malloc(size_t bytes)
{
    void *p = nullptr;
    DC_HIP_CHECK(hipMalloc(&p, bytes));
    return p;
}
void dc_free(void *dptr) { DC_HIP_CHECK(hipFree(dptr)); }
void dc_memcpy_h2d(void *dst, const void *src, size_t bytes) { DC_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); }
void dc_memcpy_d2h(void *dst, const void *src, size_t bytes) { DC_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); }
void dc_memset(void *dst, int value, size_t bytes) { DC_HIP_CHECK(hipMemset(dst, value, bytes)); }
void dc_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream)
{
    DC_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
}
void dc_stream_sync(void *stream) { DC_HIP_CHECK(hipStreamSynchronize(S(stream))); }

void dc_set_device(int device) { DC_HIP_CHECK(hipSetDevice(device)); }
void dc_device_sync(void) { DC_HIP_CHECK(hipDeviceSynchronize()); }
void dc_mem_info(uint64_t *free_bytes, uint64_t *total_bytes)
{
    size_t f = 0, t = 0;
    DC_HIP_CHECK(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
}
int dc_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

void *dc_event_create(void)
{
    hipEvent_t e;
    DC_HIP_CHECK(hipEventCreate(&e));
    return (void *)e;
}
void dc_event_destroy(void *event) { DC_HIP_CHECK(hipEventDestroy((hipEvent_t)event)); }
void dc_event_record(void *event, void *stream) { DC_HIP_CHECK(hipEventRecord((hipEvent_t)event, S(stream))); }
float dc_event_elapsed_ms(void *start, void *stop)
{
    float ms = 0.f;
    DC_HIP_CHECK(hipEventSynchronize((hipEvent_t)stop));
    DC_HIP_CHECK(hipEventElapsedTime(&ms, (hipEvent_t)start, (hipEvent_t)stop));
    return ms;
}

void dc_ntt_forward(dc_context *ctx, uint64_t *data, long limb_stride, int count, const int32_t *d_prime_idx, int prime_base,
                    int prime_period, void *stream)
{
    launch_ntt(*ctx->c, false, data, limb_stride, count, d_prime_idx, prime_base, prime_period, S(stream));
}
void dc_ntt_inverse(dc_context *ctx, uint64_t *data, long limb_stride, int count, const int32_t *d_prime_idx, int prime_base,
                    int prime_period, void *stream)
{
    launch_ntt(*ctx->c, true, data, limb_stride, count, d_prime_idx, prime_base, prime_period, S(stream));
}

// variant 0: the two-launch tiles whatever the batch size; 1: the single-crossing kernel (N = 2^15 only; aborts otherwise)
void dc_ntt_variant(dc_context *ctx, int variant, int inverse, uint64_t *data, long limb_stride, int count, const int32_t *d_prime_idx,
                    int prime_base, int prime_period, void *stream)
{
    if (variant == 1) {
        if (!ntt_full_supported(*ctx->c)) {
            fprintf(stderr, "[dacapo_amd] dc_ntt_variant: the single-crossing transform exists for N = 2^15 only\n");
            abort();
        }
        launch_ntt_full(*ctx->c, inverse != 0, data, limb_stride, count, d_prime_idx, prime_base, prime_period, S(stream));
    } else
        launch_ntt_two_phase(*ctx->c, inverse != 0, data, limb_stride, count, d_prime_idx, prime_base, prime_period, S(stream));
}

void dc_ct_negate(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *a, long a_stride, int ell, void *stream)
{
    launch_ew(*ctx->c, EwOp::Neg, V(dst, dst_stride), V(a, a_stride), V(a, a_stride), 2, 2, ell, S(stream));
}
void dc_ct_add(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *a, long a_stride, const uint64_t *b,
               long b_stride, int ell, void *stream)
{
    launch_ew(*ctx->c, EwOp::Add, V(dst, dst_stride), V(a, a_stride), V(b, b_stride), 2, 2, ell, S(stream));
}
void dc_ct_add_plain(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *a, long a_stride, const uint64_t *plain,
                     int ell, void *stream)
{
    launch_add_plain(*ctx->c, V(dst, dst_stride), V(a, a_stride), plain, ell, S(stream));
}
void dc_ct_mul_plain(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *a, long a_stride, const uint64_t *plain,
                     int ell, void *stream)
{
    launch_ew(*ctx->c, EwOp::Mul, V(dst, dst_stride), V(a, a_stride), V(plain, 0), 2, 1, ell, S(stream));
}
void dc_ct_mul_relin(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *a, long a_stride, const uint64_t *b,
                     long b_stride, const uint64_t *relin_key, int ell, void *stream)
{
    if (overlaps(dst, a) || overlaps(dst, b)) {
        mul_relin(*ctx->c, ctx->c->ws0, V(dst, dst_stride), V(a, a_stride), V(b, b_stride), relin_key, ell, S(stream));
        return;
    }
    const MulItem it{ V(a, a_stride), V(b, b_stride), V(dst, dst_stride) };
    const MulItem *d = static_cast<const MulItem *>(item_slot(ctx, &it, sizeof(it), S(stream)));
    b_mul_relin(*ctx->c, batch_ws(ctx->c->ws0), d, relin_key, 1, ell, S(stream));
}
void dc_ct_mul_relin_rescale(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *a, long a_stride, const uint64_t *b,
                             long b_stride, const uint64_t *relin_key, const uint64_t *add_plain, const uint64_t *mul_const, int ell,
                             void *stream)
{
    Context &c = *ctx->c;
    hipStream_t s = S(stream);
    if (c.hybrid()) {
        fprintf(stderr, "[dacapo_amd] dc_ct_mul_relin_rescale: this context switches keys with grouped digits, whose mod-down is an approximate base "
                        "conversion; the call is for SEAL-layout keys (use dc_ct_mul_relin and dc_ct_rescale)\n");
        abort();
    }
    if (ell < 2 || ell > c.max_level() || ell > kConstSlotWords) {
        fprintf(stderr, "[dacapo_amd] dc_ct_mul_relin_rescale: level %d (2..%d)\n", ell, std::min(c.max_level(), kConstSlotWords));
        abort();
    }
    const size_t N = c.N;
    const u64 *d_consts = nullptr;
    if (mul_const) { // the residues travel like the item: a ring of device slots written in stream order
        if (!ctx->fold_consts) DC_HIP_CHECK(hipMalloc(&ctx->fold_consts, (size_t)kItemSlots * kConstSlotWords * sizeof(u64)));
        u64 *slot = ctx->fold_consts + (size_t)(ctx->item_next % kItemSlots) * kConstSlotWords;
        DC_HIP_CHECK(hipMemcpyAsync(slot, mul_const, (size_t)ell * sizeof(u64), hipMemcpyHostToDevice, s));
        d_consts = slot;
    }
    const bool fused = mul_relin_rescale_fused(c, 1, ell), alias = overlaps(dst, a) || overlaps(dst, b);
    if (!fused || alias) {
        const size_t need = (size_t)3 * ell * N * sizeof(u64);
        if (need > ctx->fold_tmp_cap) { // (growing waits for the device: hipFree)
            if (ctx->fold_tmp) DC_HIP_CHECK(hipFree(ctx->fold_tmp));
            ctx->fold_tmp = nullptr;
            DC_HIP_CHECK(hipMalloc(&ctx->fold_tmp, need));
            ctx->fold_tmp_cap = need;
        }
    }
    if (fused) { // the last kernel's epilogue reads a and b where other workgroups write dst: an aliased destination is written through scratch
        const CtView out = alias ? CtView{ ctx->fold_tmp, (long)(ell - 1) * (long)N } : V(dst, dst_stride);
        MulRsItem it;
        it.a = V(a, a_stride), it.b = V(b, b_stride), it.dst = out;
        it.add = add_plain, it.mul = d_consts, it.mul_stride = 1;
        const MulRsItem *d = static_cast<const MulRsItem *>(item_slot(ctx, &it, sizeof(it), s));
        b_mul_relin_rescale(c, batch_ws(c.ws0), d, relin_key, 1, ell, s);
        if (alias) launch_ew(c, EwOp::Copy, V(dst, dst_stride), out, out, 2, 2, ell - 1, s);
        return;
    }
    // the default sequence (its large-batch or un-fused forms): product at level ell in scratch, then the rescale with its operand expression
    const CtView prod{ ctx->fold_tmp, (long)ell * (long)N };
    u64 *mul_plain = nullptr;
    if (d_consts) {
        mul_plain = ctx->fold_tmp + (size_t)2 * ell * N;
        fill_const_plain(c, mul_plain, d_consts, ell, s);
    }
    const MulItem mi{ V(a, a_stride), V(b, b_stride), prod };
    b_mul_relin(c, batch_ws(c.ws0), static_cast<const MulItem *>(item_slot(ctx, &mi, sizeof(mi), s)), relin_key, 1, ell, s);
    const RsItem ri{ prod, V(dst, dst_stride), 0, 0, add_plain, mul_plain };
    b_rescale(c, batch_ws(c.ws0), static_cast<const RsItem *>(item_slot(ctx, &ri, sizeof(ri), s)), 1, ell, s);
}
void dc_ct_mul(dc_context *ctx, uint64_t *dst3, long dst_stride, const uint64_t *a, long a_stride, const uint64_t *b, long b_stride, int ell,
               void *stream)
{
    launch_tensor(*ctx->c, V(dst3, dst_stride), dst3 + 2 * dst_stride, V(a, a_stride), V(b, b_stride), ell, S(stream));
}
void dc_ct_relin(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *src3, long src_stride, const uint64_t *relin_key, int ell,
                 void *stream)
{
    keyswitch(*ctx->c, ctx->c->ws0, V(dst, dst_stride), src3, src3 + src_stride, src3 + 2 * src_stride, relin_key, ell, S(stream));
}
// dst = relin(sum_k signs[k] as[k] (x) bs[k]) with one key-switch sequence (batch_ops.hip b_mul_sum_relin).  The table -- the item, then its
// terms -- is kept in the handle and copied as dc_ct_rotate_sum_hoisted copies its own.
void dc_ct_mul_sum_relin(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *const *as, const uint64_t *const *bs, const int32_t *signs,
                         int count, long src_stride, const uint64_t *relin_key, int ell, void *stream)
{
    Context &c = *ctx->c;
    hipStream_t s = S(stream);
    if (c.hybrid()) {
        fprintf(stderr, "[dacapo_amd] dc_ct_mul_sum_relin: this context switches keys with grouped digits (ks_special > 1); the call is for "
                        "SEAL-layout keys (use dc_ct_mul_relin and dc_ct_add)\n");
        abort();
    }
    if (count < 1 || count > kMulSumMax || ell < 1 || ell > c.max_level()) {
        fprintf(stderr, "[dacapo_amd] dc_ct_mul_sum_relin: %d products at level %d (1..%d products, level 1..%d)\n", count, ell, kMulSumMax,
                c.max_level());
        abort();
    }
    const size_t N = c.N;
    bool alias = false;
    for (int k = 0; k < count; k++) {
        if (signs[k] != 1 && signs[k] != -1) {
            fprintf(stderr, "[dacapo_amd] dc_ct_mul_sum_relin: sign %d of product %d (+1 or -1)\n", (int)signs[k], k);
            abort();
        }
        alias = alias || overlaps(dst, as[k]) || overlaps(dst, bs[k]);
    }
    if (alias) { // the last kernel reads the operands where other workgroups write dst: such a destination is written through scratch
        const size_t need = (size_t)2 * ell * N * sizeof(u64);
        if (need > ctx->fold_tmp_cap) { // (growing waits for the device: hipFree)
            if (ctx->fold_tmp) DC_HIP_CHECK(hipFree(ctx->fold_tmp));
            ctx->fold_tmp = nullptr;
            DC_HIP_CHECK(hipMalloc(&ctx->fold_tmp, need));
            ctx->fold_tmp_cap = need;
        }
    }
    const CtView out = alias ? CtView{ ctx->fold_tmp, (long)ell * (long)N } : V(dst, dst_stride);
    constexpr size_t kTermsAt = 64; // the item, then the terms
    static_assert(sizeof(MulSumItem) <= kTermsAt && kTermsAt % alignof(MulTerm) == 0, "product-sum table layout");
    std::vector<char> h(kTermsAt + (size_t)count * sizeof(MulTerm));
    const MulSumItem item{ out, 0, count };
    memcpy(h.data(), &item, sizeof(item));
    for (int k = 0; k < count; k++) {
        const MulTerm t{ V(as[k], src_stride), V(bs[k], src_stride), (int)signs[k] };
        memcpy(h.data() + kTermsAt + (size_t)k * sizeof(MulTerm), &t, sizeof(t));
    }
    if (h.size() > ctx->mulsum_cap) {
        if (ctx->mulsum_table) DC_HIP_CHECK(hipFree(ctx->mulsum_table));
        ctx->mulsum_table = nullptr;
        DC_HIP_CHECK(hipMalloc(&ctx->mulsum_table, kTermsAt + (size_t)kMulSumMax * sizeof(MulTerm)));
        ctx->mulsum_cap = kTermsAt + (size_t)kMulSumMax * sizeof(MulTerm);
    }
    DC_HIP_CHECK(hipMemcpyAsync(ctx->mulsum_table, h.data(), h.size(), hipMemcpyHostToDevice, s));
    DC_HIP_CHECK(hipStreamSynchronize(s)); // (the host table goes out of scope)
    const char *d = static_cast<const char *>(ctx->mulsum_table);
    b_mul_sum_relin(c, batch_ws(c.ws0), reinterpret_cast<const MulSumItem *>(d), reinterpret_cast<const MulTerm *>(d + kTermsAt), relin_key, 1, ell, s);
    if (alias) launch_ew(c, EwOp::Copy, V(dst, dst_stride), out, out, 2, 2, ell, s);
}
void dc_ct_rotate_hop(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *src, long src_stride,
                      uint32_t galois_elt, const uint64_t *galois_key, int ell, void *stream)
{
    if (overlaps(dst, src)) {
        rotate_hop(*ctx->c, ctx->c->ws0, V(dst, dst_stride), V(src, src_stride), galois_elt, galois_key, ell, S(stream));
        return;
    }
    const KsItem it{ V(src, src_stride), V(dst, dst_stride), galois_key, galois_elt, 0 };
    const KsItem *d = static_cast<const KsItem *>(item_slot(ctx, &it, sizeof(it), S(stream)));
    b_rotate_hops(*ctx->c, batch_ws(ctx->c->ws0), d, 1, ell, S(stream));
}
// dst = apply_galois(src) + addend: dc_ct_rotate_hop with one addend at level ell, which the fused middle adds exactly (KsItem::add; fused_ks.hip
// f_ks_frows_mac_kernel).  The addend is read by the middle launch alone, before the last launch writes dst: it may be src or dst.
void dc_ct_rotate_hop_add(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *src, long src_stride, const uint64_t *addend,
                          long addend_stride, uint32_t galois_elt, const uint64_t *galois_key, int ell, void *stream)
{
    if (ctx->c->hybrid()) {
        fprintf(stderr, "[dacapo_amd] dc_ct_rotate_hop_add: this context switches keys with grouped digits (ks_special > 1); the call is for "
                        "SEAL-layout keys (use dc_ct_rotate_hop and dc_ct_add)\n");
        abort();
    }
    KsItem it{ V(src, src_stride), V(dst, dst_stride), galois_key, galois_elt, 0 };
    it.add = V(addend, addend_stride);
    const KsItem *d = static_cast<const KsItem *>(item_slot(ctx, &it, sizeof(it), S(stream)));
    b_rotate_hops(*ctx->c, batch_ws(ctx->c->ws0), d, 1, ell, S(stream), Handoff{}, 0, true);
}
// `count` hops of one source on one decomposition (hoist_ks.hip).  The decomposition lives in the context's default workspace (one source);
// what grows with the hop count -- the item table, the accumulators, the mod-down terms -- is kept in the handle.
void dc_ct_rotate_hoisted(dc_context *ctx, uint64_t *const *dsts, long dst_stride, const uint64_t *src, long src_stride,
                          const uint32_t *galois_elts, const uint64_t *const *galois_keys, int count, int ell, void *stream)
{
    const size_t B = (size_t)count;
    const KsItem *d = hoist_items(ctx, "dc_ct_rotate_hoisted", ", where dc_ct_rotate_hop already takes the digits before the automorphism", "hops",
                                  count, ell, B, S(stream), [&](std::vector<KsItem> &h) {
                                      for (size_t b = 0; b < B; b++)
                                          h.push_back(KsItem{ V(src, src_stride), V(dsts[b], dst_stride), galois_keys[b], galois_elts[b], 0 });
                                      h.push_back(KsItem{ V(src, src_stride), V(src, src_stride), nullptr, 1u, 0 }); // the source, for the decomposition's loader
                                      return (size_t)0;
                                  });
    Context &c = *ctx->c;
    const BatchWs w{ c.ws0.ct_tmp, c.ws0.ks_digits, c.ws0.ks_ext, ctx->hoist_acc, ctx->hoist_tmp };
    hoist_rotate_hops(c, w, d, d + B, count, 1, ell, S(stream));
}
// dst = sum_k [plains[k] .] galois_k(srcs[k]) with ONE division by P (hoist_ks.hip hoist_rotate_sum): equal source pointers share a
// decomposition, which is why the decompositions need scratch of their own here ([distinct sources][l][N] digits and [..][l*l][N] lifted limbs,
// kept in the handle like the rest).
// addend: a ciphertext added to the sum exactly by the inner-product launch (the group's src field, hoist_ks.hip f_ks_gsum_kernel ADDEND), or null
static void rotate_sum_hoisted(dc_context *ctx, const char *who, uint64_t *dst, long dst_stride, const uint64_t *addend, long addend_stride,
                               const uint64_t *const *srcs, long src_stride, const uint32_t *galois_elts, const uint64_t *const *galois_keys,
                               const uint64_t *const *plains, const uint64_t *const *plains_sp, int count, int ell, void *stream)
{
    const size_t B = (size_t)count;
    size_t U = 0;
    const KsItem *d = hoist_items(ctx, who, " (ks_special > 1)", "members", count, ell, 1, S(stream), [&](std::vector<KsItem> &h) {
        // members source-major (stable: equal sources keep the caller's order); then the group; then the distinct sources
        std::vector<size_t> order(B);
        for (size_t b = 0; b < B; b++) order[b] = b;
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return srcs[x] < srcs[y]; });
        std::vector<KsItem> sources;
        for (size_t b : order) {
            const u64 *pl = plains ? plains[b] : nullptr, *psp = plains_sp ? plains_sp[b] : nullptr;
            if ((pl == nullptr) != (psp == nullptr)) {
                fprintf(stderr, "[dacapo_amd] %s: member %zu has one of plains / plains_sp only\n", who, b);
                abort();
            }
            const CtView sv = V(srcs[b], src_stride);
            if (sources.empty() || sources.back().src.p != sv.p) sources.push_back(KsItem{ sv, sv, nullptr, 1u, 0 });
            h.push_back(KsItem{ sv, V(dst, dst_stride), galois_keys[b], galois_elts[b], (u32)(sources.size() - 1), pl, psp });
        }
        h.push_back(KsItem{ addend ? V(addend, addend_stride) : V(dst, dst_stride), V(dst, dst_stride), nullptr, 0u, (u32)B });
        h.insert(h.end(), sources.begin(), sources.end());
        return U = sources.size();
    });
    const BatchWs w{ nullptr, ctx->hoist_digits, ctx->hoist_ext, ctx->hoist_acc, ctx->hoist_tmp };
    hoist_rotate_sum(*ctx->c, w, d, d + B + 1, count, (int)U, d + B, 1, ell, S(stream), addend != nullptr);
}
void dc_ct_rotate_sum_hoisted(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *const *srcs, long src_stride,
                              const uint32_t *galois_elts, const uint64_t *const *galois_keys, const uint64_t *const *plains,
                              const uint64_t *const *plains_sp, int count, int ell, void *stream)
{
    rotate_sum_hoisted(ctx, "dc_ct_rotate_sum_hoisted", dst, dst_stride, nullptr, 0, srcs, src_stride, galois_elts, galois_keys, plains, plains_sp,
                       count, ell, stream);
}
// ... plus `addend`, a ciphertext at level ell that the same launches add exactly (NULL: dc_ct_rotate_sum_hoisted itself)
void dc_ct_rotate_sum_hoisted_add(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *addend, long addend_stride,
                                  const uint64_t *const *srcs, long src_stride, const uint32_t *galois_elts, const uint64_t *const *galois_keys,
                                  const uint64_t *const *plains, const uint64_t *const *plains_sp, int count, int ell, void *stream)
{
    rotate_sum_hoisted(ctx, "dc_ct_rotate_sum_hoisted_add", dst, dst_stride, addend, addend_stride, srcs, src_stride, galois_elts, galois_keys,
                       plains, plains_sp, count, ell, stream);
}
void dc_ct_rescale(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *src, long src_stride, int ell, void *stream)
{
    const RsItem it{ V(src, src_stride), V(dst, dst_stride), 0, 0, nullptr, nullptr }; // element-wise epilogue: in place is fine
    const RsItem *d = static_cast<const RsItem *>(item_slot(ctx, &it, sizeof(it), S(stream)));
    b_rescale(*ctx->c, batch_ws(ctx->c->ws0), d, 1, ell, S(stream));
}
void dc_ct_modswitch(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *src, long src_stride, int ell, int down,
                     void *stream)
{
    if (down <= 0 || (dst == src && dst_stride == src_stride)) return; // dropping limbs in place moves nothing
    launch_ew(*ctx->c, EwOp::Copy, V(dst, dst_stride), V(src, src_stride), V(src, src_stride), 2, 2, ell - down, S(stream));
}

void dc_keyswitch(dc_context *ctx, uint64_t *out, long out_stride, const uint64_t *base0, const uint64_t *base1,
                  const uint64_t *target, const uint64_t *key, int ell, void *stream)
{
    keyswitch(*ctx->c, ctx->c->ws0, V(out, out_stride), base0, base1, target, key, ell, S(stream));
}
void dc_galois_ntt(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *src, long src_stride, uint32_t galois_elt,
                   int polys, int ell, void *stream)
{
    launch_galois(*ctx->c, V(dst, dst_stride), V(src, src_stride), galois_elt, polys, ell, S(stream));
}
void dc_poly_mul(dc_context *ctx, uint64_t *dst, const uint64_t *a, const uint64_t *b, int ell, void *stream)
{
    launch_ew(*ctx->c, EwOp::Mul, V(dst, 0), V(a, 0), V(b, 0), 1, 1, ell, S(stream));
}
void dc_poly_add(dc_context *ctx, uint64_t *dst, const uint64_t *a, const uint64_t *b, int ell, void *stream)
{
    launch_ew(*ctx->c, EwOp::Add, V(dst, 0), V(a, 0), V(b, 0), 1, 1, ell, S(stream));
}

// Error statistics of D = m got - want per polynomial (noise_stats.hip): the launches do not depend on `count`; the records are copied to the
// host and the call waits for them.
void dc_poly_error_stats(dc_context *ctx, const uint64_t *got, long got_stride, const uint64_t *want, long want_stride, int ell, int count,
                         int lift_prime, dc_error_stats *out_host, void *stream)
{
    static_assert(sizeof(dc_error_stats) == sizeof(NoiseStats) && offsetof(dc_error_stats, max_abs_lo) == offsetof(NoiseStats, max_lo) &&
                      offsetof(dc_error_stats, inconsistent) == offsetof(NoiseStats, inconsistent),
                  "dc_error_stats is the device record");
    Context &c = *ctx->c;
    hipStream_t s = S(stream);
    const long need = (long)ell * (long)c.N;
    if (count < 1 || count > 65535 || ell < 1 || ell > c.K || lift_prime < -1 || lift_prime >= c.K) {
        fprintf(stderr, "[dacapo_amd] dc_poly_error_stats: %d polynomials of %d limbs, lift_prime %d (1..65535 polynomials, 1..%d limbs, lift_prime -1 "
                        "or a prime index up to %d)\n", count, ell, lift_prime, c.K, c.K - 1);
        abort();
    }
    auto bad = [&](const uint64_t *p, long stride) { return ((uintptr_t)p & 15) != 0 || (stride & 1) != 0 || (count > 1 && stride < need); };
    if (!got || !out_host || bad(got, got_stride) || (want && bad(want, want_stride))) {
        fprintf(stderr, "[dacapo_amd] dc_poly_error_stats: needs polynomials and an output, 16-byte aligned, at even strides of at least ell * N = %ld "
                        "words (strides %ld, %ld)\n", need, got_stride, want_stride);
        abort();
    }
    const size_t bytes = noise_scratch_words(c, ell, count) * sizeof(u64);
    if (bytes > ctx->noise_cap) { // (growing waits for the device: hipFree)
        if (ctx->noise_buf) DC_HIP_CHECK(hipFree(ctx->noise_buf));
        ctx->noise_buf = nullptr, ctx->noise_cap = 0;
        DC_HIP_CHECK(hipMalloc(&ctx->noise_buf, bytes));
        ctx->noise_cap = bytes;
    }
    const NoiseStats *total = noise_error_stats(c, ctx->noise_buf, got, got_stride, want, want_stride, ell, count, lift_prime, s);
    DC_HIP_CHECK(hipMemcpyAsync(out_host, total, (size_t)count * sizeof(NoiseStats), hipMemcpyDeviceToHost, s));
    DC_HIP_CHECK(hipStreamSynchronize(s));
}

uint32_t dc_galois_elt_from_step(const dc_context *ctx, int step)
{
    const uint32_t n = (uint32_t)ctx->c->N, m = 2 * n;
    if (step == 0) return m - 1;
    const uint32_t pos = (uint32_t)(step < 0 ? -step : step);
    if (pos >= (n >> 1)) return 0;
    uint32_t e = step < 0 ? (n >> 1) - pos : pos;
    uint64_t elt = 1, g = 3; // 3^e mod 2N by square and multiply
    for (; e; e >>= 1) {
        if (e & 1) elt = (elt * g) & (m - 1);
        g = (g * g) & (m - 1);
    }
    return (uint32_t)elt;
}

} // extern "C"
