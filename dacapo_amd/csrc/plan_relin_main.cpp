// Stand-alone driver of the grouping pass of lazy relinearisation (plan_relin.cpp) for tests/test_plan_relin.py: built with
// AddressSanitizer + UBSan (make plan_relin_asan), no device code.  Reads a .hevm program (wire_parse.cpp), walks it as the plan does --
// registers renamed to the ops that wrote them, levels by the reference's semantics per opcode, the value a result register names when the
// program ends is a result -- and prints the groups:
//   usage : plan_relin_asan PROGRAM.hevm [CAP]          (CAP: products per group, default the kernel's kMulSumMax = 32)
//   out   : "products P groups G saved S" and per group "group closing C level L :" followed by "+M" / "-M" per product (instruction indices)
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "plan_relin.hpp"
#include "wire_parse.hpp"

using namespace dacapo;

int main(int argc, char **argv)
{
    if (argc < 2 || argc > 3) {
        fprintf(stderr, "usage: %s PROGRAM.hevm [CAP]\n", argv[0]);
        return 2;
    }
    const int cap = argc == 3 ? atoi(argv[2]) : 32;
    if (cap < 2) {
        fprintf(stderr, "plan_relin_main: a group holds at least 2 products (CAP %d)\n", cap);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    std::vector<char> raw;
    char buf[1 << 16];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) raw.insert(raw.end(), buf, buf + got);
    fclose(f);
    // (setscale names a constant of the .cst file, which plays no part here: every index holds a scale)
    const std::vector<std::vector<double>> constants(65536, std::vector<double>(1, 1.0));
    wire::Program pr;
    std::string err;
    if (!wire::parse_program(raw.data(), raw.size(), false, constants, pr, err)) {
        fprintf(stderr, "plan_relin_main: %s\n", err.c_str());
        return 2;
    }
    const size_t nreg = pr.cipher_registers, nops = pr.ops.size();
    std::vector<int> cur(nreg, -1), in_level(nreg, 0); // register -> op that wrote it (-1: a program input, at in_level)
    for (size_t i = 0; i < pr.arg_level.size() && i < nreg; i++) in_level[i] = (int)pr.arg_level[i];
    std::vector<int> kind(nops, RELIN_OTHER), src0(nops, -1), src1(nops, -1), readers(nops, 0), level(nops, 0), result(nops, 0);
    int products = 0;
    for (size_t i = 0; i < nops; i++) {
        const WireOp &op = pr.ops[i];
        const bool unary = op.opcode == 1 || op.opcode == 2 || op.opcode == 3 || op.opcode == 4 || op.opcode == 7 || op.opcode == 9 || op.opcode == 10 ||
                           (op.opcode >= kOpConj && op.opcode <= kOpKeySwitch);
        const bool binary = op.opcode == 6 || op.opcode == 8;
        if (!unary && !binary) continue; // encodes, upscale, no-ops: no cipher register changes hands
        if (op.opcode == 4 && (int16_t)op.rhs <= 0) continue; // a zero modswitch leaves dst untouched
        auto read = [&](uint16_t r, int &src) {
            src = cur[r];
            if (src >= 0) readers[(size_t)src]++;
            return src >= 0 ? level[(size_t)src] : in_level[r];
        };
        const int la = read(op.lhs, src0[i]);
        if (binary) (void)read(op.rhs, src1[i]);
        switch (op.opcode) {
        case 2: kind[i] = RELIN_NEGATE, level[i] = la; break;
        case 3: level[i] = la - 1; break;
        case 4: level[i] = la - (int16_t)op.rhs; break;
        case 6: kind[i] = RELIN_ADDCC, level[i] = la; break;
        case 8: kind[i] = RELIN_MULCC, level[i] = la, products++; break;
        case 10: level[i] = op.rhs; break;
        case kOpModRaise: level[i] = op.rhs; break;
        default: level[i] = la; break;
        }
        cur[op.dst] = (int)i;
    }
    for (uint64_t r : pr.res_dst)
        if (cur[(size_t)r] >= 0) result[(size_t)cur[(size_t)r]] = 1;
    RelinOps in;
    in.n = (int)nops, in.kind = kind.data(), in.src0 = src0.data(), in.src1 = src1.data(), in.readers = readers.data(), in.level = level.data();
    in.result = result.data();
    const std::vector<RelinGroup> groups = plan_relin_groups(in, cap);
    int saved = 0;
    for (const RelinGroup &g : groups) saved += (int)g.members.size() - 1;
    printf("products %d groups %zu saved %d\n", products, groups.size(), saved);
    for (const RelinGroup &g : groups) {
        printf("group closing %d level %d :", g.closing_op, level[(size_t)g.members[0].mul_op]);
        for (const RelinMember &m : g.members) printf(" %c%d", m.sign > 0 ? '+' : '-', m.mul_op);
        printf("\n");
    }
    return 0;
}
