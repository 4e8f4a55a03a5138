// The dataflow walk of a loaded program (plan_flow.hpp).  Host-only C++.
#include "plan_flow.hpp"

namespace dacapo {

PlanFlow plan_flow(const WireOp *ops, size_t nops, size_t nreg, const uint64_t *res_dst, size_t n_res, const uint64_t *arg_level, size_t n_args)
{
    PlanFlow f;
    f.defines.assign(nops, 0), f.src0.assign(nops, kFlowNoValue), f.src1.assign(nops, kFlowNoValue);
    f.readers.assign(nops, 0), f.result.assign(nops, 0), f.level.assign(nops, 0);
    std::vector<int> cur(nreg); // register -> the value it names
    for (size_t r = 0; r < nreg; r++) cur[r] = -1 - (int)r;
    for (size_t i = 0; i < nops; i++) {
        const WireOp &op = ops[i];
        const bool unary = op.opcode == 1 || op.opcode == 2 || op.opcode == 3 || op.opcode == 4 || op.opcode == 7 || op.opcode == 9 || op.opcode == 10 ||
                           (op.opcode >= kOpConj && op.opcode <= kOpKeySwitch);
        const bool binary = op.opcode == 6 || op.opcode == 8;
        if (!unary && !binary) continue;                                          // encodes, upscale, no-ops: no cipher register changes hands
        if (op.opcode == 4 && (int16_t)op.rhs <= 0) continue;                     // a zero modswitch leaves dst untouched
        if (op.opcode == 1 && (int16_t)op.rhs == 0 && op.dst == op.lhs) continue; // ... and so does a rotation by 0 onto itself
        if (op.lhs >= nreg || op.dst >= nreg || (binary && op.rhs >= nreg)) continue; // (whoever loaded the program has checked the operands)
        auto read = [&](uint16_t r, int &src) { // the level of what register r names
            src = cur[r];
            if (src >= 0) f.readers[(size_t)src]++;
            return src >= 0 ? f.level[(size_t)src] : r < n_args ? (int)arg_level[r] : 0;
        };
        const int la = read(op.lhs, f.src0[i]);
        if (binary) (void)read(op.rhs, f.src1[i]);
        switch (op.opcode) {
        case 3: f.level[i] = la - 1; break;                // rescale
        case 4: f.level[i] = la - (int16_t)op.rhs; break;  // modswitch
        case 10: f.level[i] = op.rhs; break;               // bootstrap: to the level it names
        case kOpModRaise: f.level[i] = op.rhs; break;
        default: f.level[i] = la; break;
        }
        f.defines[i] = 1;
        cur[op.dst] = (int)i;
    }
    for (size_t k = 0; k < n_res; k++)
        if (res_dst[k] < nreg && cur[(size_t)res_dst[k]] >= 0) f.result[(size_t)cur[(size_t)res_dst[k]]] = 1;
    return f;
}

std::vector<RelinGroup> flow_relin_groups(const PlanFlow &flow, const WireOp *ops, int cap)
{
    const size_t n = flow.defines.size();
    std::vector<int> kind(n, RELIN_OTHER);
    for (size_t i = 0; i < n; i++)
        if (flow.defines[i]) kind[i] = ops[i].opcode == 8 ? RELIN_MULCC : ops[i].opcode == 6 ? RELIN_ADDCC : ops[i].opcode == 2 ? RELIN_NEGATE : RELIN_OTHER;
    RelinOps in;
    in.n = (int)n, in.kind = kind.data(), in.src0 = flow.src0.data(), in.src1 = flow.src1.data(), in.readers = flow.readers.data();
    in.level = flow.level.data(), in.result = flow.result.data();
    return plan_relin_groups(in, cap);
}

std::vector<FlattenGroup> flow_flatten_groups(const PlanFlow &flow, const WireOp *ops, int f, int slots, const int *keyed, int n_keyed)
{
    const size_t n = flow.defines.size();
    std::vector<int> kind(n, FLAT_OTHER), offset(n, 0);
    for (size_t i = 0; i < n; i++) {
        if (!flow.defines[i]) continue;
        if (ops[i].opcode == 1) kind[i] = FLAT_ROTATE, offset[i] = (int16_t)ops[i].rhs;
        if (ops[i].opcode == 6) kind[i] = FLAT_ADDCC;
    }
    FlattenOps in;
    in.n = (int)n, in.kind = kind.data(), in.src0 = flow.src0.data(), in.src1 = flow.src1.data(), in.offset = offset.data();
    in.readers = flow.readers.data(), in.result = flow.result.data();
    return plan_flatten_groups(in, f, slots, keyed, n_keyed);
}

} // namespace dacapo
