// Stand-alone driver of the levelling pass (plan_levels.cpp) for tests/test_plan_levels.py: built with AddressSanitizer + UBSan
// (make plan_levels_asan), no device code.  Reads DAGs from a text file and prints the waves the pass gives them:
//   file  := count { dag }
//   dag   := n mode { kind level target cap fixed launches link_prev asap nprod prod* }      (n operations, program order)
//   out   := per dag three lines: "moved M steps S waves W multi X links L launches N" / "wave w0 w1 ..." / "how h0 h1 ..."
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "plan_levels.hpp"

static int next_int(FILE *f)
{
    int v;
    if (fscanf(f, "%d", &v) != 1) {
        fprintf(stderr, "plan_levels_main: truncated input\n");
        exit(2);
    }
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s DAGS.txt\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    const int count = next_int(f);
    for (int d = 0; d < count; d++) {
        const int n = next_int(f), mode = next_int(f);
        if (n < 0 || n > (1 << 24)) return 2;
        std::vector<int> kind((size_t)n), level((size_t)n), target((size_t)n), cap((size_t)n), fixed((size_t)n), launches((size_t)n), link_prev((size_t)n),
            asap((size_t)n), first((size_t)n + 1, 0), prod;
        for (int i = 0; i < n; i++) {
            const size_t k = (size_t)i;
            kind[k] = next_int(f), level[k] = next_int(f), target[k] = next_int(f), cap[k] = next_int(f), fixed[k] = next_int(f);
            launches[k] = next_int(f), link_prev[k] = next_int(f), asap[k] = next_int(f);
            const int np = next_int(f);
            for (int j = 0; j < np; j++) {
                const int p = next_int(f);
                if (p < 0 || p >= i) {
                    fprintf(stderr, "plan_levels_main: dag %d op %d names producer %d (program order is a topological order)\n", d, i, p);
                    return 2;
                }
                prod.push_back(p);
            }
            if (link_prev[k] >= i || link_prev[k] < -1) return 2;
            first[k + 1] = (int)prod.size();
        }
        dacapo::LevelOps in;
        in.n = n, in.kind = kind.data(), in.level = level.data(), in.target = target.data(), in.cap = cap.data(), in.fixed = fixed.data();
        in.launches = launches.data(), in.prod_first = first.data(), in.prod = prod.data(), in.link_prev = link_prev.data(), in.asap = asap.data();
        std::vector<int> wave((size_t)n), how((size_t)n);
        const int moved = dacapo::plan_levels(in, mode, wave.data(), how.data());
        const dacapo::LevelStats st = dacapo::plan_level_stats(in, wave.data());
        printf("moved %d steps %d waves %d multi %d links %d launches %d\nwave", moved, st.steps, st.waves, st.multi_waves, st.links, st.launches);
        for (int v : wave) printf(" %d", v);
        printf("\nhow");
        for (int v : how) printf(" %d", v);
        printf("\n");
    }
    fclose(f);
    return 0;
}
