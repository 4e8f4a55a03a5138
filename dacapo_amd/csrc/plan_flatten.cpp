// The flattening pass of rotate-and-add chains (plan_flatten.hpp).  Host-only C++.
#include "plan_flatten.hpp"

#include <algorithm>

namespace dacapo {

int flatten_norm_offset(long offset, int slots)
{
    long v = offset % slots;
    if (v > slots / 2) v -= slots;
    if (v <= -(long)(slots / 2)) v += slots;
    return (int)v;
}

std::vector<FlattenGroup> plan_flatten_groups(const FlattenOps &in, int f, int slots, const int *keyed, int n_keyed)
{
    std::vector<FlattenGroup> out;
    const size_t n = in.n > 0 ? (size_t)in.n : 0;
    if (f < 2 || slots < 2) return out;
    f = std::min(f, kFlattenMaxHops);
    // hop_rot[i] >= 0: addcc i closes a hop whose rotation is op hop_rot[i] and whose y is value hop_src[i]
    std::vector<int> hop_rot(n, -1), hop_src(n, 0), next(n, -1);
    std::vector<char> continues(n, 0); // hop i continues the chain of another hop
    auto rotation_of = [&](int a, int y) -> int { // a, if it is a single-use, unobservable rotation of y made before its reader
        if (a < 0 || in.kind[(size_t)a] != FLAT_ROTATE) return -1;
        return (in.src0[(size_t)a] == y && in.readers[(size_t)a] == 1 && !in.result[(size_t)a]) ? a : -1;
    };
    for (size_t i = 0; i < n; i++) {
        if (in.kind[i] != FLAT_ADDCC) continue;
        const int p = in.src0[i], q = in.src1[i];
        if ((p >= 0 && (size_t)p >= i) || (q >= 0 && (size_t)q >= i)) continue; // (not a topological order: no hop)
        int r = rotation_of(q, p), y = p;
        if (r < 0) r = rotation_of(p, q), y = q;
        if (r < 0) continue;
        hop_rot[i] = r, hop_src[i] = y;
        // y is the result of an earlier hop that nothing else reads (its two readers are then this rotation and this addcc)
        if (y >= 0 && hop_rot[(size_t)y] >= 0 && in.readers[(size_t)y] == 2 && !in.result[(size_t)y]) next[(size_t)y] = (int)i, continues[i] = 1;
    }
    std::vector<int> norm;
    for (size_t head = 0; head < n; head++) {
        if (hop_rot[head] < 0 || continues[head]) continue;
        std::vector<int> chain;
        for (int i = (int)head; i >= 0; i = next[(size_t)i]) chain.push_back(i);
        const size_t m = chain.size(), stages = (m + (size_t)f - 1) / (size_t)f;
        size_t at = 0;
        for (size_t s = 0; s < stages; s++) {
            const size_t h = m / stages + (s < m % stages ? 1 : 0);
            const size_t first = at;
            at += h;
            if (h < 2) continue;
            FlattenGroup g;
            g.closing_op = chain[first + h - 1], g.source = hop_src[(size_t)chain[first]];
            for (size_t k = 0; k < h; k++) g.add_ops.push_back(chain[first + k]), g.rot_ops.push_back(hop_rot[(size_t)chain[first + k]]);
            bool ok = true;
            for (unsigned mask = 1; mask < (1u << h) && ok; mask++) {
                long sum = 0;
                for (size_t k = 0; k < h; k++)
                    if (mask >> k & 1) sum += in.offset[(size_t)g.rot_ops[k]];
                const int o = flatten_norm_offset(sum, slots);
                ok = o != 0 && (!keyed || std::binary_search(keyed, keyed + n_keyed, o));
                g.offsets.push_back(o);
            }
            if (ok) out.push_back(std::move(g));
        }
    }
    std::sort(out.begin(), out.end(), [](const FlattenGroup &a, const FlattenGroup &b) { return a.closing_op < b.closing_op; });
    return out;
}

} // namespace dacapo
