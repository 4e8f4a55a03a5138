// Stand-alone driver of the flattening pass of rotate-and-add chains (plan_flatten.cpp) for tests/test_plan_flatten.py: built with
// AddressSanitizer + UBSan (make plan_flatten_asan), no device code.  Reads a .hevm program (wire_parse.cpp), walks it as the plan does --
// registers renamed to the ops that wrote them (a program input is the value -1 - register), the value a result register names when the
// program ends is a result, a rotation by 0 onto its own register changes nothing -- and prints the groups:
//   usage : plan_flatten_asan PROGRAM.hevm F SLOTS [KEYS]
//           F: hops per stage (2 .. 6); SLOTS = N / 2; KEYS: comma-separated slot offsets that have a key (default: every offset has one)
//   out   : "rotates R groups G hops H members M offsets D composite C" -- H hops absorbed, D distinct member offsets, C of them the sum of two
//           or more hops and no single hop's of any group -- and per group
//           "group closing C source V hops H : ROT/ADD ... : OFFSET ..."     (instruction indices; V < 0: input register -1 - V)
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "plan_flatten.hpp"
#include "wire_parse.hpp"

using namespace dacapo;

int main(int argc, char **argv)
{
    if (argc < 4 || argc > 5) {
        fprintf(stderr, "usage: %s PROGRAM.hevm F SLOTS [KEYS]\n", argv[0]);
        return 2;
    }
    const int f = atoi(argv[2]), slots = atoi(argv[3]);
    if (f < 2 || f > kFlattenMaxHops || slots < 2 || (slots & (slots - 1))) {
        fprintf(stderr, "plan_flatten_main: F is 2 .. %d and SLOTS a power of two (F %d, SLOTS %d)\n", kFlattenMaxHops, f, slots);
        return 2;
    }
    std::vector<int> keyed;
    if (argc == 5) {
        for (const char *p = argv[4]; *p;) {
            char *end = nullptr;
            const long v = strtol(p, &end, 10);
            if (end == p) {
                fprintf(stderr, "plan_flatten_main: KEYS is a comma-separated list of offsets\n");
                return 2;
            }
            keyed.push_back(flatten_norm_offset(v, slots));
            p = *end == ',' ? end + 1 : end;
        }
        std::sort(keyed.begin(), keyed.end());
    }
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) {
        perror(argv[1]);
        return 2;
    }
    std::vector<char> raw;
    char buf[1 << 16];
    for (size_t got; (got = fread(buf, 1, sizeof buf, fp)) > 0;) raw.insert(raw.end(), buf, buf + got);
    fclose(fp);
    // (setscale names a constant of the .cst file, which plays no part here: every index holds a scale)
    const std::vector<std::vector<double>> constants(65536, std::vector<double>(1, 1.0));
    wire::Program pr;
    std::string err;
    if (!wire::parse_program(raw.data(), raw.size(), false, constants, pr, err)) {
        fprintf(stderr, "plan_flatten_main: %s\n", err.c_str());
        return 2;
    }
    const size_t nreg = pr.cipher_registers, nops = pr.ops.size();
    std::vector<int> cur(nreg); // register -> the value it names
    for (size_t r = 0; r < nreg; r++) cur[r] = -1 - (int)r;
    std::vector<int> kind(nops, FLAT_OTHER), src0(nops, 0), src1(nops, 0), offset(nops, 0), readers(nops, 0), result(nops, 0);
    int rotates = 0;
    for (size_t i = 0; i < nops; i++) {
        const WireOp &op = pr.ops[i];
        const bool unary = op.opcode == 1 || op.opcode == 2 || op.opcode == 3 || op.opcode == 4 || op.opcode == 7 || op.opcode == 9 || op.opcode == 10 ||
                           (op.opcode >= kOpConj && op.opcode <= kOpKeySwitch);
        const bool binary = op.opcode == 6 || op.opcode == 8;
        if (!unary && !binary) continue; // encodes, upscale, no-ops: no cipher register changes hands
        if (op.opcode == 4 && (int16_t)op.rhs <= 0) continue; // a zero modswitch leaves dst untouched
        if (op.opcode == 1) rotates++;
        if (op.opcode == 1 && (int16_t)op.rhs == 0 && op.dst == op.lhs) continue; // ... and so does a rotation by 0 onto itself
        auto read = [&](uint16_t r) {
            const int v = cur[r];
            if (v >= 0) readers[(size_t)v]++;
            return v;
        };
        src0[i] = read(op.lhs);
        if (binary) src1[i] = read(op.rhs);
        if (op.opcode == 1) kind[i] = FLAT_ROTATE, offset[i] = (int16_t)op.rhs;
        if (op.opcode == 6) kind[i] = FLAT_ADDCC;
        cur[op.dst] = (int)i;
    }
    for (uint64_t r : pr.res_dst)
        if (r < nreg && cur[(size_t)r] >= 0) result[(size_t)cur[(size_t)r]] = 1;
    FlattenOps in;
    in.n = (int)nops, in.kind = kind.data(), in.src0 = src0.data(), in.src1 = src1.data(), in.offset = offset.data(), in.readers = readers.data();
    in.result = result.data();
    const std::vector<FlattenGroup> groups = plan_flatten_groups(in, f, slots, argc == 5 ? keyed.data() : nullptr, (int)keyed.size());
    size_t hops = 0, members = 0;
    std::set<int> all, single;
    for (const FlattenGroup &g : groups) {
        hops += g.rot_ops.size(), members += g.offsets.size();
        all.insert(g.offsets.begin(), g.offsets.end());
        for (size_t k = 0; k < g.rot_ops.size(); k++) single.insert(g.offsets[((size_t)1 << k) - 1]);
    }
    size_t composite = 0;
    for (int o : all) composite += single.count(o) ? 0 : 1;
    printf("rotates %d groups %zu hops %zu members %zu offsets %zu composite %zu\n", rotates, groups.size(), hops, members, all.size(), composite);
    for (const FlattenGroup &g : groups) {
        printf("group closing %d source %d hops %zu :", g.closing_op, g.source, g.rot_ops.size());
        for (size_t k = 0; k < g.rot_ops.size(); k++) printf(" %d/%d", g.rot_ops[k], g.add_ops[k]);
        printf(" :");
        for (int o : g.offsets) printf(" %d", o);
        printf("\n");
    }
    return 0;
}
