// The kernel-level handle of include/dacapo_ckks.h: a (possibly borrowed) Context.
#pragma once
#include "context.hpp"

struct dc_context {
    dacapo::Context *c;
    bool owned; // false when the context belongs to an HEVM (hevm_context())
    void *item_ring = nullptr; // device slots for the one-item tables of the fused composite ops (c_api.hip)
    unsigned item_next = 0;
    // dc_ct_rotate_hoisted: item table [hops + 1], accumulators [hops][2][l+1][N] and mod-down terms [hops][2][l][N], grown on demand
    void *hoist_items = nullptr;
    dacapo::u64 *hoist_acc = nullptr, *hoist_tmp = nullptr;
    size_t hoist_item_cap = 0, hoist_acc_cap = 0, hoist_tmp_cap = 0;
    // dc_ct_rotate_sum_hoisted uses the same three, plus the decompositions of its distinct sources: digits [U][l][N], lifted limbs [U][l*l][N]
    dacapo::u64 *hoist_digits = nullptr, *hoist_ext = nullptr;
    size_t hoist_digits_cap = 0, hoist_ext_cap = 0;
    // dc_ct_mul_relin_rescale: a ring of mul_const residue tables, and [3][l][N] for a destination that aliases an operand / the default sequence
    dacapo::u64 *fold_consts = nullptr, *fold_tmp = nullptr;
    size_t fold_tmp_cap = 0;
    // dc_ct_mul_sum_relin: the item and its term table (a destination that aliases an operand goes through fold_tmp)
    void *mulsum_table = nullptr;
    size_t mulsum_cap = 0;
    // dc_poly_error_stats: the difference polynomials and the reduction's records (noise_stats.hpp noise_scratch_words), grown on demand
    dacapo::u64 *noise_buf = nullptr;
    size_t noise_cap = 0;
};
