// The dataflow of a loaded program, walked once for the plan's grouping passes (plan_relin.hpp, plan_flatten.hpp): cipher registers renamed
// to the instructions that wrote them, readers counted per operand slot, a value observable only through a RESULT register.  Host-only C++.
// The rules live in plan_flow.cpp and nowhere else: which opcodes read one or two cipher registers and write one, which instructions
// change nothing and are skipped, the guard of operand and result indices against the register count, the level of a result per opcode.
//
// Value ids: i >= 0 is the result of instruction i; -1 - r is what register r held before the program ran (a program input).
//
// The library walks the instructions it loaded (plan_exec.hip build_plan, hevm_vm.hip hevm_flatten_offsets) and the sanitizer-built driver
// the ones it parsed (plan_groups_main.cpp, tests/test_plan_relin.py, tests/test_plan_flatten.py) with this one function.  Nothing is kept
// between calls: the result registers can change under a loaded program (resetResDst).
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "plan_flatten.hpp"
#include "plan_relin.hpp"
#include "wire_parse.hpp"

namespace dacapo {

constexpr int kFlowNoValue = INT_MIN; // an operand slot the instruction does not have

struct PlanFlow { // per instruction, in program order
    std::vector<int> defines; // non-zero: the instruction writes a cipher value (every other field is that of "no value" otherwise)
    std::vector<int> src0;    // value id of the first operand
    std::vector<int> src1;    // ... of the second (addcc, mulcc), kFlowNoValue otherwise
    std::vector<int> readers; // operand slots of later instructions that read this value
    std::vector<int> result;  // non-zero: a result register names the value when the program ends
    std::vector<int> level;   // primes of the value
};

// nreg: cipher registers.  res_dst: the result registers, n_res of them.  arg_level: the primes of input register r, r < n_args (0 beyond).
PlanFlow plan_flow(const WireOp *ops, size_t nops, size_t nreg, const uint64_t *res_dst, size_t n_res, const uint64_t *arg_level, size_t n_args);

// The two passes on a flow: kinds (and a rotation's offset) from the opcodes, everything else as walked.
std::vector<RelinGroup> flow_relin_groups(const PlanFlow &flow, const WireOp *ops, int cap);
std::vector<FlattenGroup> flow_flatten_groups(const PlanFlow &flow, const WireOp *ops, int f, int slots, const int *keyed, int n_keyed);

} // namespace dacapo
