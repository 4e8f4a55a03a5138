// The grouping pass of lazy relinearisation (plan_relin.hpp).  Host-only C++.
#include "plan_relin.hpp"

#include <algorithm>

namespace dacapo {

std::vector<RelinGroup> plan_relin_groups(const RelinOps &in, int cap)
{
    const size_t n = in.n > 0 ? (size_t)in.n : 0;
    // leaves[i] > 0: op i heads a tree of only addcc / negate over that many qualifying products (a product heads the tree of itself)
    std::vector<int> leaves(n, 0), leaf_level(n, -1);
    std::vector<char> absorbed(n, 0); // the op is an interior node or a leaf of its reader's tree
    // operand p of op i, if it may hang below i: produced by an earlier op of the list, read by i alone, not a result, heading a tree
    auto child = [&](size_t i, int p) -> int {
        if (p < 0 || (size_t)p >= i) return -1;
        const size_t c = (size_t)p;
        return (leaves[c] > 0 && in.readers[c] == 1 && !in.result[c]) ? p : -1;
    };
    for (size_t i = 0; i < n; i++) {
        if (in.kind[i] == RELIN_MULCC) {
            leaves[i] = 1, leaf_level[i] = in.level[i];
        } else if (in.kind[i] == RELIN_NEGATE) {
            const int a = child(i, in.src0[i]);
            if (a < 0) continue;
            leaves[i] = leaves[(size_t)a], leaf_level[i] = leaf_level[(size_t)a];
            absorbed[(size_t)a] = 1;
        } else if (in.kind[i] == RELIN_ADDCC) {
            const int a = child(i, in.src0[i]), b = child(i, in.src1[i]);
            if (a < 0 || b < 0 || a == b) continue; // (a == b: two slots read it, so readers is 2 and child() said no already)
            if (leaf_level[(size_t)a] != leaf_level[(size_t)b] || leaves[(size_t)a] + leaves[(size_t)b] > cap) continue;
            leaves[i] = leaves[(size_t)a] + leaves[(size_t)b], leaf_level[i] = leaf_level[(size_t)a];
            absorbed[(size_t)a] = absorbed[(size_t)b] = 1;
        }
    }
    std::vector<RelinGroup> out;
    for (size_t r = 0; r < n; r++) {
        if (absorbed[r] || leaves[r] < 2) continue; // (a product alone, or one under negates only, stays as it is)
        RelinGroup g;
        g.closing_op = (int)r;
        std::vector<RelinMember> stack{ RelinMember{ (int)r, 1 } }; // (op, sign of the path so far)
        while (!stack.empty()) {
            const RelinMember m = stack.back();
            stack.pop_back();
            const size_t i = (size_t)m.mul_op;
            if (in.kind[i] == RELIN_MULCC) {
                g.members.push_back(m);
                continue;
            }
            g.interior.push_back(m.mul_op);
            if (in.kind[i] == RELIN_NEGATE)
                stack.push_back(RelinMember{ in.src0[i], -m.sign });
            else
                stack.push_back(RelinMember{ in.src0[i], m.sign }), stack.push_back(RelinMember{ in.src1[i], m.sign });
        }
        std::sort(g.members.begin(), g.members.end(), [](const RelinMember &x, const RelinMember &y) { return x.mul_op < y.mul_op; });
        out.push_back(std::move(g));
    }
    return out;
}

} // namespace dacapo
