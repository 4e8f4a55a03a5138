// Stand-alone driver of the key switch's launch rule (launch_shape.hpp) for tests/test_launch_shape.py: built with options.cpp under
// AddressSanitizer + UBSan (make launch_shape_asan), no device code.  Options come from DACAPO_HEVM_OPTIONS as in the library.
//   usage := launch_shape_asan { logN hybrid B ell }
//   out   := per case one line "big fused_mac folds_rescale carries_addend chain_fusion" (0 / 1 each)
#include <stdio.h>
#include <stdlib.h>

#include "launch_shape.hpp"

int main(int argc, char **argv)
{
    if (argc < 5 || (argc - 1) % 4 != 0) {
        fprintf(stderr, "usage: %s { logN hybrid B ell }\n", argv[0]);
        return 2;
    }
    for (int i = 1; i < argc; i += 4) {
        const int logN = atoi(argv[i]), hybrid = atoi(argv[i + 1]), B = atoi(argv[i + 2]), ell = atoi(argv[i + 3]);
        if (logN < 10 || logN > 17 || B < 1 || B > 65535 || ell < 1 || ell > 64) return 2;
        const dacapo::KsShape sh = dacapo::ks_shape((size_t)1 << logN, hybrid != 0, B, ell);
        printf("%d %d %d %d %d\n", (int)sh.big, (int)sh.fused_mac, (int)sh.folds_rescale(), (int)sh.carries_addend(),
               (int)dacapo::chain_fusion_supported());
    }
    return 0;
}
