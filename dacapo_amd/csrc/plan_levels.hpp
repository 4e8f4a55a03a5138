// Slack-aware levelling of the plan's pseudo-ops (option plan_level; plan_exec.hip between sections 3 and 4).  Host-only C++.
//
// The plan levels operations ASAP (wave = deepest producer + 1) and forms one step per wave and bucket (kind, level, target).  An operation
// that is not on the longest dependency chain then usually forms a one-item step of its own -- a full launch sequence -- a few waves before
// a step of the same bucket runs anyway for the critical chain.  This pass keeps every operation inside its window [ASAP, ALAP] (the depth
// does not grow) and moves one with slack to the first wave of its window that already holds a step of its bucket.  Batching moves no
// arithmetic: an item's limbs do not depend on which step carries it.
//
// The interface is plain arrays over the LIVE pseudo-ops in program order (a topological order), so the pass is built and tested without
// a GPU (plan_levels_main.cpp, tests/test_plan_levels.py).
#pragma once

namespace dacapo {

struct LevelOps {
    int n = 0;
    const int *kind = nullptr, *level = nullptr, *target = nullptr; // the bucket key: an operation joins only a bucket of its exact key
    const int *cap = nullptr;        // items one step of the operation's bucket holds (max_batch for the heavy kinds)
    const int *fixed = nullptr;      // non-zero: never moved (a P_ROTSUM group keeps its wave: its chunks are cut by member count)
    const int *launches = nullptr;   // launches of one step of the operation's kind (the cost model of the final guard)
    const int *prod_first = nullptr; // producers of operation i: prod[prod_first[i] .. prod_first[i + 1])
    const int *prod = nullptr;
    const int *link_prev = nullptr;  // the producer whose last kernel could run this operation's first phase (section 4b), or -1
    const int *asap = nullptr;       // ASAP wave, >= 1
};

struct LevelStats { // of a wave assignment, by the pass's own model of sections 4 and 4b
    int steps = 0, waves = 0, multi_waves = 0, links = 0, launches = 0;
};
LevelStats plan_level_stats(const LevelOps &in, const int *wave);

enum LevelHow : int { LEVEL_STAYED = 0, LEVEL_JOINED = 1, LEVEL_FORCED = 2 };
// mode 0: wave = asap.  mode 1: the pass.  `how` (optional, [n]): what happened to each operation -- it kept its ASAP wave, it joined a
// non-empty bucket of its key later in its window, or a moved producer pushed it to its earliest feasible wave.  Returns the number of
// operations whose wave differs from ASAP.  The result never has more steps or more launches (by plan_level_stats) than ASAP: otherwise
// ASAP is returned.
int plan_levels(const LevelOps &in, int mode, int *wave, int *how = nullptr);

} // namespace dacapo
