// Flattening pass of rotate-and-add chains (option ks_flatten_sums): which log-step slot sums of a program
//   y_0 = x,  y_{k+1} = y_k + rotate(y_k, o_k)      (k = 0 .. m - 1)
// can run as ONE hoisted lazy sum per stage (hoist_ks.hip f_ks_gsum_kernel with an addend) where the program runs m dependent key switches:
//   y_m = x + sum over the non-empty subsets S of the hops of rotate(x, sum_{k in S} o_k)
// -- 2^m - 1 rotations of one source, which share one decomposition (option ks_hoist) and one division by P (option ks_lazy_sum).  Host-only C++.
//
//   * Hop: a = rotate(y, o) followed by y' = addcc(y, a) in either operand order, where a is read once (by that addcc) and is no program
//     result.  The offset is free: the rotation is replaced, so whether it is one hop or several under the key set plays no part.
//   * Chain: continues from y' while y' is read exactly twice -- by the next hop's rotate and addcc -- and is no program result; cut where
//     this fails (a third reader, a result, a rotation read twice).
//   * Stages: a chain of m hops becomes ceil(m / f) stages whose sizes differ by at most one, the larger ones first.  A stage of h >= 2
//     hops is one group: source = the stage's first y, 2^h - 1 members with the subset sums of its offsets (member k - 1 <-> the subset whose
//     hops are the set bits of k = 1 .. 2^h - 1, bit 0 = the stage's first hop), addend = the source.  A stage of one hop stays as written.
//   * A stage is NOT flattened -- its hops run as the program wrote them -- when a non-empty subset sum is 0 modulo the slot count (that
//     member would be no rotation; two subset sums that merely coincide stay two members), or when a member's offset has no key in the
//     caller's key set.  The pass never asks for a key.
// The rounding of a group differs from its instructions' (one mod-down instead of h), so whoever applies the groups does it under an option.
// Same caveat as lazy relinearisation (plan_relin.hpp): a value counts as observable only through a RESULT register; an architectural
// register that is no result and still names an absorbed interior value (a stage's rotations, its adds but the closing one) when the program
// ends is not refreshed by a run that applies the groups.
//
// The interface is plain arrays over the ops in program order, so the pass is built and tested without a GPU (plan_groups_main.cpp,
// tests/test_plan_flatten.py); plan_flow.hpp fills them from a loaded program.
#pragma once
#include <vector>

namespace dacapo {

enum FlattenKind : int { FLAT_OTHER = 0, FLAT_ROTATE = 1, FLAT_ADDCC = 2 };
constexpr int kFlattenMaxHops = 6; // 2^6 - 1 = 63 members: what one group of f_ks_gsum_kernel walks

// Operands are VALUE ids: i >= 0 is the result of op i of the list; a negative id is any other value (a program input, a view), and two
// operands carry the same negative id exactly when they are the same value.
struct FlattenOps {
    int n = 0;
    const int *kind = nullptr;    // FlattenKind
    const int *src0 = nullptr;    // first operand (rotate: the rotated value; addcc: lhs)
    const int *src1 = nullptr;    // addcc: rhs; unused otherwise
    const int *offset = nullptr;  // rotate: signed slot offset (left = positive)
    const int *readers = nullptr; // operand slots of later ops that read this op's result
    const int *result = nullptr;  // non-zero: the result is observable when the program ends
};

struct FlattenGroup {
    int closing_op = -1;          // the stage's last addcc: the op whose result the group computes
    int source = 0;               // value id of the stage's first y: the members' source and the addend
    std::vector<int> rot_ops, add_ops; // the stage's hops in chain order; add_ops.back() == closing_op
    std::vector<int> offsets;     // the 2^h - 1 members' slot offsets, normalised into (-slots / 2, slots / 2]
};

// the representative of `offset` modulo `slots` in (-slots / 2, slots / 2] (what hevm_add_rotation_keys takes)
int flatten_norm_offset(long offset, int slots);

// Groups in the program order of their closing ops.  f: the most hops a stage absorbs, 2 .. kFlattenMaxHops (below 2: no groups).  slots = N / 2.
// keyed: the normalised offsets that have a key, ascending, n_keyed of them; nullptr: every offset has one.
std::vector<FlattenGroup> plan_flatten_groups(const FlattenOps &in, int f, int slots, const int *keyed, int n_keyed);

} // namespace dacapo
