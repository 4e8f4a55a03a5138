// Grouping pass of lazy relinearisation: which ct x ct products of a program are only ever added together, so that
//   relin(sum_k s_k a_k (x) b_k)
// can take ONE key switch (dc_ct_mul_sum_relin, batch_ops.hip b_mul_sum_relin) where n mulcc instructions take n.  Host-only C++.
//
// A group is a maximal tree over the program's SSA values whose interior nodes are addcc or negate and whose leaves are mulcc:
//   * every node below the root is read exactly once (operand slots are counted: x + x reads x twice) and is not a program result;
//   * all leaves sit at one level, there are at least two of them and at most `cap` (the kernel's term table);
//   * a leaf's sign is the parity of the negates on its path to the root.
// A tree that fails somewhere is cut there: an addcc with a bare ciphertext operand, with operands at two levels or with more than `cap`
// products below it is no interior node, and the largest qualifying subtrees under it form groups of their own (one product alone stays a
// mulcc).  The rounding of a group differs from its instructions' (one mod-down instead of n), so whoever applies the groups does it under
// an option.
//
// The interface is plain arrays over the ops in program order (a topological order), so the pass is built and tested without a GPU
// (plan_groups_main.cpp, tests/test_plan_relin.py); plan_flow.hpp fills them from a loaded program.
#pragma once
#include <vector>

namespace dacapo {

enum RelinKind : int { RELIN_OTHER = 0, RELIN_MULCC = 1, RELIN_ADDCC = 2, RELIN_NEGATE = 3 };

struct RelinOps {
    int n = 0;
    const int *kind = nullptr;    // RelinKind
    const int *src0 = nullptr;    // op that produced the first operand, negative: none of the list (a program input)
    const int *src1 = nullptr;    // ... the second operand (addcc, mulcc), negative otherwise
    const int *readers = nullptr; // operand slots of later ops that read this op's result
    const int *level = nullptr;   // primes of the op's result
    const int *result = nullptr;  // non-zero: the result is observable when the program ends
};

struct RelinMember {
    int mul_op, sign; // sign +1 / -1
};
struct RelinGroup {
    int closing_op = -1;              // the tree's root: the op whose result the group computes
    std::vector<RelinMember> members; // the products, in program order
    std::vector<int> interior;        // the addcc / negate ops of the tree, the root included: whoever applies the group drops them
};

// Groups in the program order of their closing ops.  cap >= 2.
std::vector<RelinGroup> plan_relin_groups(const RelinOps &in, int cap);

} // namespace dacapo
