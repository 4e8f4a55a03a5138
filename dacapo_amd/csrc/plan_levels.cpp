// Slack-aware levelling (plan_levels.hpp).  Host-only C++: built with the host compiler, tested without a GPU.
#include "plan_levels.hpp"

#include <algorithm>
#include <map>
#include <set>
#include <tuple>
#include <vector>

namespace dacapo {

namespace {
typedef std::tuple<int, int, int> Key;                  // (kind, level, target)
typedef std::map<int, std::vector<int>> ByWave;         // wave -> members, in the order they were placed
inline Key key_of(const LevelOps &in, int i) { return Key(in.kind[i], in.level[i], in.target[i]); }
inline int chunks(size_t count, int cap) { return (int)((count + (size_t)std::max(cap, 1) - 1) / (size_t)std::max(cap, 1)); }
} // namespace

LevelStats plan_level_stats(const LevelOps &in, const int *wave)
{
    LevelStats st;
    std::map<std::pair<int, Key>, std::vector<int>> buckets; // (wave, key) -> members: the order in which section 4 forms its steps
    for (int i = 0; i < in.n; i++) buckets[{ wave[i], key_of(in, i) }].push_back(i);
    std::map<int, int> steps_of_wave;
    std::set<std::pair<int, Key>> taken; // producer steps that already hand off to a consumer
    for (auto &kv : buckets) {
        const std::vector<int> &b = kv.second;
        const int i0 = b[0], c = chunks(b.size(), in.cap[i0]);
        st.steps += c, st.launches += c * in.launches[i0];
        steps_of_wave[kv.first.first] += c;
        st.waves = std::max(st.waves, kv.first.first);
        if (c != 1) continue;
        // section 4b's rule, step for step: every item's first-phase operand comes from ONE producer step, item for item
        bool ok = true;
        std::pair<int, Key> a;
        std::set<int> prevs;
        for (size_t k = 0; k < b.size() && ok; k++) {
            const int lp = in.link_prev[b[k]];
            if (lp < 0 || !prevs.insert(lp).second) {
                ok = false;
                break;
            }
            const std::pair<int, Key> ak{ wave[lp], key_of(in, lp) };
            if (k && ak != a) ok = false;
            a = ak;
        }
        if (!ok || taken.count(a)) continue;
        const std::vector<int> &ab = buckets.at(a);
        if (ab.size() != b.size() || chunks(ab.size(), in.cap[ab[0]]) != 1) continue;
        taken.insert(a);
        st.links++, st.launches--;
    }
    for (auto &kv : steps_of_wave) st.multi_waves += kv.second > 1;
    return st;
}

int plan_levels(const LevelOps &in, int mode, int *wave, int *how)
{
    const int n = in.n;
    for (int i = 0; i < n; i++) {
        wave[i] = in.asap[i];
        if (how) how[i] = LEVEL_STAYED;
    }
    if (mode == 0 || n == 0) return 0;
    int depth = 0;
    for (int i = 0; i < n; i++) depth = std::max(depth, in.asap[i]);
    // ALAP against the ASAP depth: a sink may wait for the last wave, a producer for the wave before its earliest consumer's latest
    std::vector<int> alap((size_t)n, depth);
    // (a fixed operation's latest wave is its ASAP wave: its producers must not move past it)
    for (int i = n - 1; i >= 0; i--) {
        if (in.fixed[i]) alap[(size_t)i] = in.asap[i];
        for (int k = in.prod_first[i]; k < in.prod_first[i + 1]; k++) alap[(size_t)in.prod[k]] = std::min(alap[(size_t)in.prod[k]], alap[(size_t)i] - 1);
    }
    std::vector<std::vector<int>> link_next((size_t)n);
    for (int i = 0; i < n; i++)
        if (in.link_prev[i] >= 0) link_next[(size_t)in.link_prev[i]].push_back(i);
    // operations without slack keep their wave and seed the buckets
    std::map<Key, ByWave> placed;
    std::vector<char> done((size_t)n, 0);
    std::vector<int> w((size_t)n), h((size_t)n, LEVEL_STAYED);
    for (int i = 0; i < n; i++) {
        w[(size_t)i] = in.asap[i];
        if (in.fixed[i] || alap[(size_t)i] <= in.asap[i]) placed[key_of(in, i)][in.asap[i]].push_back(i), done[(size_t)i] = 1;
    }
    auto has_room = [&](const std::vector<int> &b, int cap) { return !b.empty() && b.size() % (size_t)std::max(cap, 1) != 0; }; // (joining adds no chunk)
    for (int i = 0; i < n; i++) {
        if (done[(size_t)i]) continue;
        int lo = 1;
        for (int k = in.prod_first[i]; k < in.prod_first[i + 1]; k++) lo = std::max(lo, w[(size_t)in.prod[k]] + 1);
        const int hi = alap[(size_t)i];
        ByWave &mine = placed[key_of(in, i)];
        int at = -1;
        // a linkable consumer follows its producer: its producer's step-mates hand their results to a step of this key -- join that step,
        // so that the link of section 4b still finds the two steps item for item
        const int lp = in.link_prev[i];
        if (lp >= 0) {
            const std::vector<int> &mates = placed[key_of(in, lp)][w[(size_t)lp]];
            for (int m : mates)
                for (int c : link_next[(size_t)m]) {
                    if (c == i || !done[(size_t)c] || key_of(in, c) != key_of(in, i)) continue;
                    const int wc = w[(size_t)c];
                    if (wc < lo || wc > hi || (at >= 0 && wc >= at) || !has_room(mine[wc], in.cap[i])) continue;
                    at = wc;
                }
        }
        if (at < 0)
            for (auto it = mine.lower_bound(lo); it != mine.end() && it->first <= hi; ++it)
                if (has_room(it->second, in.cap[i])) {
                    at = it->first;
                    break;
                }
        h[(size_t)i] = at < 0 ? (lo == in.asap[i] ? LEVEL_STAYED : LEVEL_FORCED) : (at == in.asap[i] ? LEVEL_STAYED : LEVEL_JOINED);
        if (at < 0) at = lo;
        w[(size_t)i] = at, done[(size_t)i] = 1;
        mine[at].push_back(i);
    }
    // the guard: a producer that moved can split consumers that ASAP had in one step -- never return more steps or launches than ASAP's
    const LevelStats before = plan_level_stats(in, in.asap), after = plan_level_stats(in, w.data());
    if (after.steps > before.steps || after.launches > before.launches || after.waves > before.waves) return 0;
    int moved = 0;
    for (int i = 0; i < n; i++) {
        wave[i] = w[(size_t)i], moved += w[(size_t)i] != in.asap[i];
        if (how) how[i] = h[(size_t)i];
    }
    return moved;
}

} // namespace dacapo
