/*
 * dacapo_ckks.h -- kernel-level C ABI of the MI355X HEVM runtime (libSEAL_HEVM.so, same library that exports
 * the 18 HEVM symbols of include/hevm_abi.h).
 *
 * Each entry point stands for one call that /root/reference/lib/Runtime/SEAL_HEVM.cpp makes into Microsoft
 * SEAL 4.0.0 (the reference's FFI boundary for the arithmetic of the hot path); the citation after each
 * declaration is the reference line that makes the call.  Plain pointers and sizes only: polynomial data are
 * DEVICE pointers to uint64 limbs, `stream` is a hipStream_t (NULL = default stream).  Nothing here
 * synchronises or allocates unless it says so.  A missing GPU / failed HIP call aborts the process with a
 * message, like the reference's asserts and uncaught SEAL exceptions do (SEAL_HEVM.cpp:295,327,496).
 *
 * Layouts (limb-major, N coefficients per limb, NTT domain = SEAL's bit-reversed evaluation order):
 *   polynomial at level ell : [ell][N]                 limb i is modulo prime i of the chain
 *   ciphertext              : 2 polynomials, `poly_stride` elements apart (poly_stride >= ell*N)
 *   key-switch key          : [K-1 digits][2][K][N]    K = primes in the key-level chain, special prime = K-1
 */
#ifndef DACAPO_CKKS_H
#define DACAPO_CKKS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: what this header declares is what it exports */
#endif

typedef struct dc_context dc_context;

/* seal::EncryptionParameters + SEALContext: N = 2^logN, `num_primes` primes.  primes == NULL builds
 * CoeffModulus::Create(N, {bit_size x num_primes}) exactly as SEAL_HEVM.cpp:48-53 does (bit_size must be 60:
 * the HIP reduction is specialised to q = 2^60 - delta, delta < 2^28).  Uploads twiddle tables.  Synchronous. */
dc_context *dc_context_create(int logN, int num_primes, int bit_size, const uint64_t *primes);
/* EXTENSION (not SEAL's scheme; the reference's HEaaN runtime has it inside its closed library, HEAAN_HEVM.cpp:124-141): key switching
 * with grouped digits -- the last `special` primes of the chain are special, a decomposition digit is a group of `alpha` data primes
 * (alpha <= special), key-switch keys are [dc_context_key_digits()][2][K][N] and data levels run up to dc_context_max_level() =
 * num_primes - special.  special = alpha = 1 is dc_context_create's (SEAL's) scheme. */
dc_context *dc_context_create_hybrid(int logN, int num_primes, int special, int alpha);
/* ... on an explicit prime chain (each prime 2^b - d as for dc_context_create; widths other than 60 bits: libSEAL_HEVM_gw.so) */
dc_context *dc_context_create_hybrid_primes(int logN, const uint64_t *primes, int num_primes, int special, int alpha);
int dc_context_key_digits(const dc_context *ctx);
int dc_context_max_level(const dc_context *ctx);
void dc_context_destroy(dc_context *ctx);
int dc_context_logn(const dc_context *ctx);
int dc_context_num_primes(const dc_context *ctx);
void dc_context_primes(const dc_context *ctx, uint64_t *out /* [num_primes] host */);
void dc_context_roots(const dc_context *ctx, uint64_t *out /* [num_primes] host: minimal primitive 2N-th roots */);

/* device memory plumbing so that callers need no HIP/torch types (all synchronous) */
void *dc_malloc(size_t bytes);
void dc_free(void *dptr);
void dc_memcpy_h2d(void *dst, const void *src, size_t bytes);
void dc_memcpy_d2h(void *dst, const void *src, size_t bytes);
void dc_memset(void *dst, int value, size_t bytes);
void dc_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream); /* asynchronous on `stream` */
void dc_stream_sync(void *stream);
void dc_set_device(int device);  /* hipSetDevice: one process per GPU, call before creating contexts/VMs */
void dc_device_sync(void);       /* hipDeviceSynchronize */
int dc_device_count(void);
/* free and total HBM of the current device in bytes (hipMemGetInfo) */
void dc_mem_info(uint64_t *free_bytes, uint64_t *total_bytes);
/* HIP events on `stream`, for timing the kernels where they are launched (bench.py) */
void *dc_event_create(void);
void dc_event_destroy(void *event);
void dc_event_record(void *event, void *stream);
float dc_event_elapsed_ms(void *start, void *stop); /* synchronises on `stop` */

/* util::ntt_negacyclic_harvey / inverse_ntt_negacyclic_harvey over `count` limbs at data + b*limb_stride, in place.
 * Limb b is modulo prime d_prime_idx[b] (DEVICE int32 array) or, if NULL, prime_base + (b % prime_period)
 * (prime_period <= 0: prime_base + b).  Reached from every rotate/rescale/mulcc/encode of SEAL_HEVM.cpp
 * (:262,:273,:283,:316). */
void dc_ntt_forward(dc_context *ctx, uint64_t *data, long limb_stride, int count, const int32_t *d_prime_idx, int prime_base,
                    int prime_period, void *stream);
void dc_ntt_inverse(dc_context *ctx, uint64_t *data, long limb_stride, int count, const int32_t *d_prime_idx, int prime_base,
                    int prime_period, void *stream);

/* The same transform with the implementation named (tests and bench.py compare them; dc_ntt_forward/inverse choose by batch size):
 * variant 0 = two launches per transform (ntt_tile.hpp), 1 = one 1024-thread workgroup per limb, one HBM crossing (ntt_full.hip,
 * N = 2^15 only). */
void dc_ntt_variant(dc_context *ctx, int variant, int inverse, uint64_t *data, long limb_stride, int count, const int32_t *d_prime_idx,
                    int prime_base, int prime_period, void *stream);

/* Evaluator::negate            SEAL_HEVM.cpp:278 */
void dc_ct_negate(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *a, long a_stride, int ell, void *stream);
/* Evaluator::add               SEAL_HEVM.cpp:302 */
void dc_ct_add(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *a, long a_stride, const uint64_t *b,
               long b_stride, int ell, void *stream);
/* Evaluator::add_plain         SEAL_HEVM.cpp:309 */
void dc_ct_add_plain(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *a, long a_stride, const uint64_t *plain,
                     int ell, void *stream);
/* Evaluator::multiply_plain    SEAL_HEVM.cpp:322 */
void dc_ct_mul_plain(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *a, long a_stride, const uint64_t *plain,
                     int ell, void *stream);
/* Evaluator::multiply + relinearize_inplace   SEAL_HEVM.cpp:315-316 */
void dc_ct_mul_relin(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *a, long a_stride, const uint64_t *b,
                     long b_stride, const uint64_t *relin_key, int ell, void *stream);
/* Evaluator::multiply alone: the three-part product, polynomials `dst_stride` apart in dst3 -- d0 = a0 b0, d1 = a0 b1 + a1 b0, d2 = a1 b1
 * (oracle Oracle.tensor).  dst3 must not overlap a or b. */
void dc_ct_mul(dc_context *ctx, uint64_t *dst3, long dst_stride, const uint64_t *a, long a_stride, const uint64_t *b, long b_stride, int ell,
               void *stream);
/* Evaluator::relinearize_inplace of a three-part ciphertext (polynomials `src_stride` apart): dst = (d0, d1) + KS(d2), dc_keyswitch's path,
 * so either key mode.  dst may be src3 (in place).  dc_ct_relin(dc_ct_mul(a, b)) equals dc_ct_mul_relin(a, b) limb for limb. */
void dc_ct_relin(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *src3, long src_stride, const uint64_t *relin_key, int ell,
                 void *stream);
/* EXTENSION (not SEAL's rounding for count > 1): dst = relinearize(sum_k signs[k] * as[k] (x) bs[k]) with ONE key-switch sequence -- the
 * launches of one dc_ct_mul_relin whatever the count.  The three-part sum T = sum_k signs[k] * Oracle.tensor(as[k], bs[k]) is formed in exact
 * modular arithmetic (poly_add / poly_sub), then dst = (T0, T1) + KS(T2), limb for limb Oracle.keyswitch(T2, relin, T0, T1); count = 1 with
 * sign +1 is dc_ct_mul_relin exactly.  as / bs: HOST arrays of `count` device pointers to ciphertexts of poly stride `src_stride`; signs: HOST
 * array of +1 / -1.  1 <= count <= DC_CT_MUL_SUM_MAX; more aborts with a message (split the sum and dc_ct_add the parts).  as[k] may equal bs[k]
 * (a square), an operand may appear in several terms, dst may be an operand (it is then written through scratch and copied: one more launch).
 * SEAL-layout contexts only (a grouped-digit context aborts with a message).  Scratch is kept in the context.  The item table is copied
 * synchronously: the call waits for earlier work on `stream`. */
#define DC_CT_MUL_SUM_MAX 32
void dc_ct_mul_sum_relin(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *const *as, const uint64_t *const *bs,
                         const int32_t *signs, int count, long src_stride, const uint64_t *relin_key, int ell, void *stream);
/* Evaluator::multiply + relinearize_inplace [+ add_plain + multiply_plain by a constant polynomial] + rescale_to_next, limb for limb;
 * dst at level ell-1.  add_plain: [>= ell][N] NTT form or NULL.  mul_const: HOST array of ell residues (the constant polynomial's value
 * modulo each prime) or NULL.  ell >= 2.  dst may be a or b; a may be b.  SEAL-layout contexts only.
 * The rescale is folded into the multiply's key switch: ONE exact pass divides by P q_{ell-1} (five launches instead of seven, ell-1 forward
 * transforms per polynomial instead of 2 ell-1) and every limb equals dc_ct_mul_relin [+ dc_ct_add_plain + dc_ct_mul_plain] + dc_ct_rescale.
 * Launch shapes without a folded form (options ks_big_tiles, ks_fuse_mac, ks_fuse_mac_tiles) run that default sequence instead.  A
 * grouped-digit context aborts with a message: its mod-down is an approximate base conversion.  Scratch is kept in the context. */
void dc_ct_mul_relin_rescale(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *a, long a_stride, const uint64_t *b,
                             long b_stride, const uint64_t *relin_key, const uint64_t *add_plain, const uint64_t *mul_const, int ell,
                             void *stream);
/* Evaluator::apply_galois_inplace: one hop of Evaluator::rotate_vector   SEAL_HEVM.cpp:273 */
void dc_ct_rotate_hop(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *src, long src_stride,
                      uint32_t galois_elt, const uint64_t *galois_key, int ell, void *stream);
/* EXTENSION: dc_ct_rotate_hop plus one addend -- dst = apply_galois(src) + addend, the addend (a ciphertext of ell limbs, NTT form) added
 * EXACTLY and with no launch of its own: it enters the key switch's accumulators of the data primes as P . addend, which the division by P
 * returns unchanged, so every limb equals Oracle.add(Oracle.apply_galois(src, elt), addend).  addend may be src or dst (it is read before dst
 * is written); dst must not be src.  SEAL-layout contexts only (a grouped-digit context aborts with a message), and only where the key
 * switch's middle is one launch (options ks_fuse_mac, ks_fuse_mac_tiles: otherwise the call aborts with a message).  y' = y + rotate(y, o)
 * is one such call (option ks_fold_add). */
void dc_ct_rotate_hop_add(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *src, long src_stride, const uint64_t *addend,
                          long addend_stride, uint32_t galois_elt, const uint64_t *galois_key, int ell, void *stream);
/* EXTENSION (not SEAL's rounding): `count` hops of ONE source ciphertext sharing one decomposition -- the digits of c1 are taken before the
 * automorphism (inverse NTT, every digit lifted to every modulus, forward NTT: once per call) and each hop reads them through its Galois
 * permutation: oracle orc_rotate_ks_hybrid at one special prime / one prime per digit, limb for limb, for every count.  dsts / elts / keys:
 * host arrays of length count; keys in dc_ct_rotate_hop's layout.  A dst may be src; the dsts must be distinct.  SEAL-layout contexts only
 * (a grouped-digit context aborts with a message: its dc_ct_rotate_hop already hoists).  Scratch is kept in the context, sized on first use.
 * The item table is copied synchronously: the call waits for earlier work on `stream`. */
void dc_ct_rotate_hoisted(dc_context *ctx, uint64_t *const *dsts, long dst_stride, const uint64_t *src, long src_stride,
                          const uint32_t *galois_elts, const uint64_t *const *galois_keys, int count, int ell, void *stream);
/* EXTENSION (not SEAL's rounding): dst = sum_k [plains[k] .] galois_k(srcs[k]) with ONE division by P -- the members' inner products (and
 * their base terms) are added in the raised basis, a member with a plaintext multiplied by it there, and the sum is brought down once: per
 * member oracle orc_rotate_acc_hybrid at one special prime / one prime per digit, Oracle.lazy_mul_plain / lazy_add, then one
 * orc_moddown_hybrid, limb for limb.  srcs / elts / keys / plains / plains_sp: host arrays of length count.  plains[k]: the plaintext's limbs
 * over the data primes [>= ell][N], plains_sp[k]: the same encoded polynomial's limb at the special prime [N], both NTT form (both or neither);
 * either array may be NULL altogether and single entries may be NULL: a bare term.  Equal srcs pointers share one decomposition; dst may be one
 * of the sources.  SEAL-layout contexts only (a grouped-digit context aborts with a message).  Scratch is kept in the context, sized on
 * first use.  The item table is copied synchronously: the call waits for earlier work on `stream`. */
void dc_ct_rotate_sum_hoisted(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *const *srcs, long src_stride,
                              const uint32_t *galois_elts, const uint64_t *const *galois_keys, const uint64_t *const *plains,
                              const uint64_t *const *plains_sp, int count, int ell, void *stream);
/* EXTENSION: dc_ct_rotate_sum_hoisted plus one addend -- dst = addend + sum_k [plains[k] .] galois_k(srcs[k]), the addend (a ciphertext of ell
 * limbs, NTT form) added EXACTLY and with no launch of its own: it enters the raised accumulators of the data primes as P . addend, which the
 * one division by P returns unchanged, so every limb equals Oracle.add(addend, the sum without it).  addend may be one of the sources, may be
 * dst, or NULL (then the call is dc_ct_rotate_sum_hoisted).  Everything else as there.  y + rot(y, a) + rot(y, b) + rot(y, a + b) -- two hops
 * of a rotate-and-add chain -- is one such call with three members (option ks_flatten_sums). */
void dc_ct_rotate_sum_hoisted_add(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *addend, long addend_stride,
                                  const uint64_t *const *srcs, long src_stride, const uint32_t *galois_elts,
                                  const uint64_t *const *galois_keys, const uint64_t *const *plains, const uint64_t *const *plains_sp,
                                  int count, int ell, void *stream);
/* Evaluator::rescale_to_next: level ell -> ell-1   SEAL_HEVM.cpp:283 */
void dc_ct_rescale(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *src, long src_stride, int ell,
                   void *stream);
/* Evaluator::mod_switch_to_next (CKKS: drop the last `down` limbs = copy the kept ones)   SEAL_HEVM.cpp:289-291 */
void dc_ct_modswitch(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *src, long src_stride, int ell, int down,
                     void *stream);

/* building blocks exposed for the parity tests */
/* Evaluator::switch_key_inplace: (out0,out1) = (base0,base1) + KS(target); base pointers may be NULL (= 0). */
void dc_keyswitch(dc_context *ctx, uint64_t *out, long out_stride, const uint64_t *base0, const uint64_t *base1,
                  const uint64_t *target, const uint64_t *key, int ell, void *stream);
/* GaloisTool::apply_galois_ntt on `polys` polynomials of `ell` limbs */
void dc_galois_ntt(dc_context *ctx, uint64_t *dst, long dst_stride, const uint64_t *src, long src_stride, uint32_t galois_elt,
                   int polys, int ell, void *stream);
/* limb-wise dyadic product / sum of two [ell][N] polynomials (dyadic_product_coeffmod / add_poly_coeffmod) */
void dc_poly_mul(dc_context *ctx, uint64_t *dst, const uint64_t *a, const uint64_t *b, int ell, void *stream);
void dc_poly_add(dc_context *ctx, uint64_t *dst, const uint64_t *a, const uint64_t *b, int ell, void *stream);

/* EXTENSION (measurement, not an operation of the scheme): how far `got` is from `want`, as exact integers.  got / want hold `count`
 * polynomials [ell][N] in NTT form, got_stride / want_stride words apart (even, >= ell * N; the pointers 16-byte aligned); want == NULL
 * stands for 0.  D = m got - want over limbs 0 .. ell-1, with m = 1 when lift_prime is -1 and m = q_{lift_prime} (taken modulo every limb)
 * otherwise -- the rescale case: got the result at ell primes, want the operand's first ell limbs, lift_prime >= ell the dropped prime, so
 * that D / m is the rounding error.  lift_prime < ell is allowed too: m is 0 modulo that limb, so got's limb there is not read into D and D
 * is -want on it -- a rescale's result padded with one zero limb against the WHOLE operand, which is how a rescale to one prime is
 * measured (q_1 . out - in exceeds q_0 / 2, but not q_0 q_1 / 2).  Every coefficient of D is lifted to the centred integer it stands for in
 * (-M/2, M/2], M = q_0 at ell = 1 and q_0 q_1 otherwise (|D| must stay below M/2: the further limbs are only checked against that value
 * and disagreements counted in `inconsistent`).  One record per polynomial is written to out_host[count] (HOST memory); the call
 * synchronises `stream`.  Launches: the difference, the batched inverse transform, lift-and-reduce, finish -- the same number whatever
 * `count` is; no atomics, so equal inputs give equal bits on every run.  Scratch is kept in the context.
 * noise, in the unit of the reference compiler's noiseTable, is (N/2) mean_j (D_j / m)^2 = sum_sq / 2. */
typedef struct {
    double sum_sq;                   /* sum_j (D_j / m)^2 */
    double sum;                      /* sum_j  D_j / m    */
    uint64_t max_abs_lo, max_abs_hi; /* max_j |D_j|, exact, 128 bits */
    int64_t inconsistent;            /* coefficients whose further limbs contradict the value lifted from the first two */
} dc_error_stats;
void dc_poly_error_stats(dc_context *ctx, const uint64_t *got, long got_stride, const uint64_t *want, long want_stride, int ell, int count,
                         int lift_prime, dc_error_stats *out_host, void *stream);

/* GaloisTool::get_elt_from_step (host): step > 0 rotates left; 0 = conjugation; returns 0 if |step| >= N/2 */
uint32_t dc_galois_elt_from_step(const dc_context *ctx, int step);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
