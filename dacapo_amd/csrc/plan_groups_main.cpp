// Stand-alone driver of the plan's two grouping passes -- lazy relinearisation (plan_relin.cpp) and the flattening of rotate-and-add chains
// (plan_flatten.cpp) -- for tests/test_plan_relin.py and tests/test_plan_flatten.py: built with AddressSanitizer + UBSan (make
// plan_groups_asan), no device code.  Reads a .hevm program (wire_parse.cpp), walks it with the library's own walk (plan_flow.cpp) and
// prints the groups:
//   usage : plan_groups_asan relin PROGRAM.hevm [CAP]            (CAP: products per group, default the kernel's kMulSumMax = 32)
//   out   : "products P groups G saved S" and per group "group closing C level L :" followed by "+M" / "-M" per product (instruction indices)
//   usage : plan_groups_asan flatten PROGRAM.hevm F SLOTS [KEYS]
//           F: hops per stage (2 .. 6); SLOTS = N / 2; KEYS: comma-separated slot offsets that have a key (default: every offset has one)
//   out   : "rotates R groups G hops H members M offsets D composite C" -- H hops absorbed, D distinct member offsets, C of them the sum of two
//           or more hops and no single hop's of any group -- and per group
//           "group closing C source V hops H : ROT/ADD ... : OFFSET ..."     (instruction indices; V < 0: input register -1 - V)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "plan_flow.hpp"

using namespace dacapo;

int main(int argc, char **argv)
{
    const bool relin = argc >= 2 && !strcmp(argv[1], "relin"), flatten = argc >= 2 && !strcmp(argv[1], "flatten");
    if (!(relin && argc >= 3 && argc <= 4) && !(flatten && argc >= 5 && argc <= 6)) {
        fprintf(stderr, "usage: %s relin PROGRAM.hevm [CAP]\n       %s flatten PROGRAM.hevm F SLOTS [KEYS]\n", argv[0], argv[0]);
        return 2;
    }
    const char *who = relin ? "plan_groups_main relin" : "plan_groups_main flatten";
    const int cap = relin && argc == 4 ? atoi(argv[3]) : 32;
    if (cap < 2) {
        fprintf(stderr, "%s: a group holds at least 2 products (CAP %d)\n", who, cap);
        return 2;
    }
    const int f = flatten ? atoi(argv[3]) : 2, slots = flatten ? atoi(argv[4]) : 2;
    if (f < 2 || f > kFlattenMaxHops || slots < 2 || (slots & (slots - 1))) {
        fprintf(stderr, "%s: F is 2 .. %d and SLOTS a power of two (F %d, SLOTS %d)\n", who, kFlattenMaxHops, f, slots);
        return 2;
    }
    std::vector<int> keyed;
    if (argc == 6) {
        for (const char *p = argv[5]; *p;) {
            char *end = nullptr;
            const long v = strtol(p, &end, 10);
            if (end == p) {
                fprintf(stderr, "%s: KEYS is a comma-separated list of offsets\n", who);
                return 2;
            }
            keyed.push_back(flatten_norm_offset(v, slots));
            p = *end == ',' ? end + 1 : end;
        }
        std::sort(keyed.begin(), keyed.end());
    }
    FILE *fp = fopen(argv[2], "rb");
    if (!fp) {
        perror(argv[2]);
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
        fprintf(stderr, "%s: %s\n", who, err.c_str());
        return 2;
    }
    const PlanFlow flow =
        plan_flow(pr.ops.data(), pr.ops.size(), pr.cipher_registers, pr.res_dst.data(), pr.res_dst.size(), pr.arg_level.data(), pr.arg_level.size());
    auto count = [&](uint16_t opcode) { return (int)std::count_if(pr.ops.begin(), pr.ops.end(), [&](const WireOp &op) { return op.opcode == opcode; }); };
    if (relin) {
        const std::vector<RelinGroup> groups = flow_relin_groups(flow, pr.ops.data(), cap);
        int saved = 0;
        for (const RelinGroup &g : groups) saved += (int)g.members.size() - 1;
        printf("products %d groups %zu saved %d\n", count(8), groups.size(), saved);
        for (const RelinGroup &g : groups) {
            printf("group closing %d level %d :", g.closing_op, flow.level[(size_t)g.members[0].mul_op]);
            for (const RelinMember &m : g.members) printf(" %c%d", m.sign > 0 ? '+' : '-', m.mul_op);
            printf("\n");
        }
        return 0;
    }
    const std::vector<FlattenGroup> groups = flow_flatten_groups(flow, pr.ops.data(), f, slots, argc == 6 ? keyed.data() : nullptr, (int)keyed.size());
    size_t hops = 0, members = 0;
    std::set<int> all, single;
    for (const FlattenGroup &g : groups) {
        hops += g.rot_ops.size(), members += g.offsets.size();
        all.insert(g.offsets.begin(), g.offsets.end());
        for (size_t k = 0; k < g.rot_ops.size(); k++) single.insert(g.offsets[((size_t)1 << k) - 1]);
    }
    size_t composite = 0;
    for (int o : all) composite += single.count(o) ? 0 : 1;
    printf("rotates %d groups %zu hops %zu members %zu offsets %zu composite %zu\n", count(1), groups.size(), hops, members, all.size(), composite);
    for (const FlattenGroup &g : groups) {
        printf("group closing %d source %d hops %zu :", g.closing_op, g.source, g.rot_ops.size());
        for (size_t k = 0; k < g.rot_ops.size(); k++) printf(" %d/%d", g.rot_ops[k], g.add_ops[k]);
        printf(" :");
        for (int o : g.offsets) printf(" %d", o);
        printf("\n");
    }
    return 0;
}
